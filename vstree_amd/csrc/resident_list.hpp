// What the handles that post-process match lists share beyond
// search_host.hpp (select.hip, cluster.hip, matchcluster.hip with
// matchcluster_erate.inc, chain.hip): the list that accumulates in HBM over
// the calls of _add, the gate in front of _add, the count of the records a
// kernel refuses, the delivery of chosen records, and the layout in device
// memory.  Everything here is inline or a template; nothing instantiates
// rocPRIM.
#ifndef VSA_RESIDENT_LIST_HPP
#define VSA_RESIDENT_LIST_HPP
#include "search_host.hpp"

// ---- the list --------------------------------------------------------------------

// n records so far in room for `capacity`: the records with their D/P flags
// (unless `records` is off: the edges of one finish), and up to MAXCOLUMNS
// side columns, which the owner keeps as typed pointers of its own and names
// here by their address.
struct ResidentList
{
  enum
  {
    MAXCOLUMNS = 3
  };
  struct Column
  {
    void **p;
    uint32_t per, size; // elements per record, bytes per element
  };
  int device = 0;
  uint64_t n = 0, capacity = 0;
  bool records = true;
  vsa_match *recs = nullptr;
  uint8_t *flags = nullptr;
  Column col[MAXCOLUMNS];
  int ncol = 0;

  template <typename T>
  void column(T **p, uint32_t per = 1)
  {
    col[ncol].p = (void **) p;
    col[ncol].per = per;
    col[ncol].size = (uint32_t) sizeof(T);
    ncol++;
  }
  // room for `need` records; what is there stays.  Array by array (one wait
  // each, the old and the new block of one array at a time): where a later one
  // fails, the earlier ones are larger than `capacity` says, which stays right
  int reserve(uint64_t need)
  {
    if (need <= capacity)
    {
      return 0;
    }
    const uint64_t cap = std::max<uint64_t>(need, 2 * capacity);
    if (records && (grow((void **) &recs, n, cap, sizeof(vsa_match)) != 0 ||
                    grow((void **) &flags, n, cap, 1) != 0))
    {
      return -100;
    }
    for (int q = 0; q < ncol; q++)
    {
      if (grow(col[q].p, col[q].per * n, col[q].per * cap, col[q].size) != 0)
      {
        return -100;
      }
    }
    capacity = cap;
    return 0;
  }
  // (the device of the list is the current one)
  void release()
  {
    vsa_dev_free(recs);
    vsa_dev_free(flags);
    recs = nullptr;
    flags = nullptr;
    for (int q = 0; q < ncol; q++)
    {
      vsa_dev_free(*col[q].p);
      *col[q].p = nullptr;
    }
    n = capacity = 0;
  }
};

// ---- the gate of _add ------------------------------------------------------------

// the rule most handles have for the form of a list
inline const char *selfform(int kind, int palindromic)
{
  return palindromic && kind == VSA_SINK_SELF
             ? "palindromic self matches are the selfpalindromic form"
             : nullptr;
}

// What every _add checks before it looks at a record, in this order: the
// arguments, a packed result, the form of the list (form() gives the text of
// the handle's own refusal, or null), the device, the room for the records
// (limit 0: none here) and enter().  `noun` and `doing` are the handle's
// words for its messages ("chain", "chaining"), `limitwords` those of the
// limit.  Below 0: refused; 1: an empty list, nothing to do; 0: go on.
template <class H, class Form>
int gate(const char *who, const char *noun, const char *doing, const H *c,
         const vsa_result *r, Form form, uint64_t limit,
         const char *limitwords)
{
  if (c == nullptr || r == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  if (r->packbits != 0)
  {
    VSA_ERROR("%s: a packed candidate result has no records to %s", who, noun);
    return VSA_NOT_COVERED;
  }
  if (r->extended)
  {
    VSA_ERROR("%s: lists of extended seeds (VSA_SINK_QUERY_HAMMING, "
              "VSA_SINK_SELF_HAMMING, VSA_SINK_QUERY_EDIST, "
              "VSA_SINK_SELF_EDIST) are not covered", who);
    return VSA_NOT_COVERED;
  }
  const char *refusal = form();
  if (refusal != nullptr)
  {
    VSA_ERROR("%s: %s", who, refusal);
    return VSA_NOT_COVERED;
  }
  if (r->device != c->device)
  {
    VSA_ERROR("%s: result on device %d, %s on device %d", who, r->device,
              doing, c->device);
    return -2;
  }
  if (limit != 0 && c->list.n + r->count >= limit)
  {
    VSA_ERROR("%s: %lu %s are covered", who,
              (unsigned long) (c->list.n + r->count), limitwords);
    return VSA_NOT_COVERED;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  return r->count == 0 ? 1 : 0;
}

// the gate of what a finished handle delivers; H::finishname is its _finish
template <class H>
int needfinished(const H *c, const char *who)
{
  if (c == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  if (!c->finished)
  {
    VSA_ERROR("%s: %s has not seen the last list", who, H::finishname);
    return -2;
  }
  return 0;
}

// ---- the records a kernel refuses --------------------------------------------------

// *counter += the lanes of the wavefront whose flag is set: one atomic per
// wavefront that has any.  Every lane of the wavefront that is still in the
// kernel calls it.
__device__ __forceinline__ void wave_count(bool flag,
                                           unsigned long long *counter)
{
  const unsigned long long b = __ballot(flag);
  if (b != 0 && (threadIdx.x & 63u) == (uint32_t) (__ffsll(b) - 1))
  {
    atomicAdd(counter, (unsigned long long) __popcll(b));
  }
}

// a few 64-bit words in device memory which a kernel counts or reduces into
struct ScratchWords
{
  DevBuf d;
  int alloc(int nwords)
  {
    return d.alloc((size_t) nwords * 8);
  }
  unsigned long long *word(int q)
  {
    return d.as<unsigned long long>() + q;
  }
  int zero(int first, int count) // in stream order
  {
    VSA_HIP(hipMemsetAsync(word(first), 0, (size_t) count * 8, nullptr));
    return 0;
  }
  int fetch(int first, int count, uint64_t *out) // waits for the stream
  {
    VSA_HIP(hipMemcpy(out, word(first), (size_t) count * 8,
                      hipMemcpyDeviceToHost));
    return 0;
  }
};

// (what the kernel wrote for such a list lies behind the records that count)
inline int misfits(const char *who, uint64_t nbad, const char *which)
{
  VSA_ERROR("%s: %lu records do not fit the layout (%s)", who,
            (unsigned long) nbad, which);
  return -2;
}

// ---- delivery --------------------------------------------------------------------

// out[t] = in[order[t]], whatever G::move makes of it
template <class G>
__global__ void __launch_bounds__(VSA_BLOCK)
k_cl_gather(G g, const uint32_t *__restrict__ order, uint64_t n)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    g.move(t, order[t]);
  }
}

// a record and its D/P flag
struct RecGather
{
  const vsa_match *recs;
  const uint8_t *flags;
  vsa_match *outrecs;
  uint8_t *outflags;

  __device__ void move(uint64_t t, uint32_t i) const
  {
    outrecs[t] = recs[i];
    outflags[t] = flags[i];
  }
};

// the records order[0 .. k) of the list (device memory) as a result of their
// own, their flags to palindromic[] (host, or null).  `span`, if there is
// one, stops behind the gather.  (A template, as members_to_host() is: only a
// translation unit that delivers records gets the gather kernel.)
template <class L>
int records_of(const L &l, const uint32_t *order, uint64_t k,
                      uint8_t *palindromic, Timer *span, vsa_result **out)
{
  vsa_result *res = newresult(l.device);
  ResultGuard guard = {res};
  if (k > 0)
  {
    DevBuf oflags;
    if (oflags.alloc(k) != 0 ||
        vsa_dev_alloc((void **) &res->matches, k * sizeof(vsa_match)) != 0)
    {
      return -100;
    }
    const RecGather g = {l.recs, l.flags, res->matches, oflags.as<uint8_t>()};
    k_cl_gather<RecGather><<<gridfor(k), VSA_BLOCK, 0, nullptr>>>(g, order, k);
    VSA_HIP(hipGetLastError());
    if (span != nullptr)
    {
      span->stop();
    }
    VSA_HIP(hipStreamSynchronize(nullptr));
    if (palindromic != nullptr)
    {
      VSA_HIP(hipMemcpy(palindromic, oflags.p, k, hipMemcpyDeviceToHost));
    }
    res->count = k;
    res->stats.count = k;
    if (sumlengths(res->matches, k, nullptr, &res->stats.sumlength) != 0)
    {
      return -100;
    }
  }
  guard.r = nullptr;
  *out = res;
  return 0;
}

// the records order[0 .. k) of the list into host memory
template <class L>
int members_to_host(const L &l, const uint32_t *order,
                           uint64_t k, std::vector<vsa_match> &out)
{
  out.resize(k);
  if (k > 0)
  {
    DevBuf drecs, dflags;
    if (drecs.alloc(k * sizeof(vsa_match)) != 0 || dflags.alloc(k) != 0)
    {
      return -100;
    }
    const RecGather g = {l.recs, l.flags, drecs.as<vsa_match>(),
                         dflags.as<uint8_t>()};
    k_cl_gather<RecGather><<<gridfor(k), VSA_BLOCK, 0, nullptr>>>(g, order, k);
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(out.data(), drecs.p, k * sizeof(vsa_match),
                      hipMemcpyDeviceToHost));
  }
  return 0;
}

// ---- the layout in device memory ---------------------------------------------------

// the query Multiseq and the separator positions of a handle's rules
struct DeviceLayout
{
  int device = 0;
  uint64_t *d_qstart = nullptr, *d_qlen = nullptr, *d_markpos = nullptr;

  // upload_queryview(), and (*markpos)[0 .. nmark) likewise (qstart or
  // markpos null: the handle has none)
  int upload(const char *who, uint64_t nq, const uint64_t **qstart,
             const uint64_t **qlen, uint64_t nmark, const uint64_t **markpos)
  {
    if (qstart != nullptr &&
        upload_queryview(nq, qstart, qlen, &d_qstart, &d_qlen, who) != 0)
    {
      return -100;
    }
    if (markpos == nullptr)
    {
      return 0;
    }
    if (nmark > 0 &&
        (vsa_hip_malloc((void **) &d_markpos, nmark * 8) != hipSuccess ||
         hipMemcpy(d_markpos, *markpos, nmark * 8, hipMemcpyHostToDevice) !=
             hipSuccess))
    {
      VSA_ERROR("%s: upload of the separator positions failed", who);
      return -100;
    }
    *markpos = d_markpos;
    return 0;
  }
  void release()
  {
    (void) hipSetDevice(device);
    (void) hipFree(d_qstart);
    (void) hipFree(d_qlen);
    (void) hipFree(d_markpos);
    d_qstart = d_qlen = d_markpos = nullptr;
  }
};

#endif
