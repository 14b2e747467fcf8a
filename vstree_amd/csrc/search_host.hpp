// Host-side helpers shared by the translation units of the search engine
// (esa_search.hip, selfmum_search.hip, approx_entry.hip, selfmatch_entry.hip,
// candidate_partition.hip, index_derive.hip, index_build.hip) and of the
// handles that post-process match lists (coverage.hip, and through
// resident_list.hpp select.hip, cluster.hip, matchcluster.hip, chain.hip).
// Small things are inline here; what
// instantiates rocPRIM is defined once, in search_common.hip.  (rocprim_run()
// is a template over its caller's lambda: it instantiates nothing of rocPRIM
// by itself.)
#ifndef VSA_SEARCH_HOST_HPP
#define VSA_SEARCH_HOST_HPP
#include <cstring>
#include <algorithm>
#include "esa_device.hpp"

#define VSA_BLOCK 256
#define VSA_CURSOR_STRIDE 8   // uint64 words: one cursor per 64-byte line
#define VSA_CURSOR_SHARDS 2048 // power of two
#define VSA_HIDDEN __attribute__((visibility("hidden")))

struct DevBuf
{
  void *p = nullptr;
  ~DevBuf()
  {
    vsa_dev_free(p);
  }
  void free()
  {
    vsa_dev_free(p);
    p = nullptr;
  }
  int alloc(size_t bytes)
  {
    free();
    return vsa_dev_alloc(&p, bytes > 0 ? bytes : 16);
  }
  template <typename T>
  T *as()
  {
    return (T *) p;
  }
  void *release()
  {
    void *r = p;
    p = nullptr;
    return r;
  }
};

// p[0 .. have) moves into a block of `cap` elements of `size` bytes
inline int grow(void **p, uint64_t have, uint64_t cap, size_t size)
{
  DevBuf b;
  if (b.alloc(cap * size) != 0)
  {
    return -100;
  }
  if (have > 0)
  {
    VSA_HIP(hipMemcpyAsync(b.p, *p, have * size, hipMemcpyDeviceToDevice,
                           nullptr));
    VSA_HIP(hipStreamSynchronize(nullptr));
  }
  vsa_dev_free(*p);
  *p = b.release();
  return 0;
}

struct Timer
{
  hipEvent_t a = nullptr, b = nullptr;
  hipStream_t s;
  bool started = false, stopped = false;
  explicit Timer(hipStream_t stream) : s(stream)
  {
    (void) hipEventCreate(&a);
    (void) hipEventCreate(&b);
  }
  ~Timer()
  {
    (void) hipEventDestroy(a);
    (void) hipEventDestroy(b);
  }
  void start()
  {
    started = hipEventRecord(a, s) == hipSuccess;
  }
  void stop()
  {
    stopped = hipEventRecord(b, s) == hipSuccess;
  }
  double ms() // after the stream has been synchronised
  {
    // a timer that never ran must not leave an error behind: the runtime
    // keeps the last error, and the next library call would report it
    float f = 0;
    if (!started || !stopped ||
        hipEventElapsedTime(&f, a, b) != hipSuccess)
    {
      (void) hipGetLastError();
      return 0.0;
    }
    return (double) f;
  }
};

// Small results the host needs before it can go on (counts, maxima) come
// back through a page of pinned memory: a device-to-host copy into pageable
// memory is staged by the runtime and costs 30-150 us each, several times
// per batch.  The page lives as long as the thread (never freed: the runtime
// may be gone when thread-local destructors run).
struct Fetch
{
  const void *src;
  size_t bytes; // <= 8
};

// (search_common.hip)
VSA_HIDDEN int fetchwords(hipStream_t stream, const Fetch *items, int count,
                          uint64_t *out);

// A rocPRIM algorithm, called the rocPRIM way: once for the size of its
// scratch space, which temp then holds, once to do the work.
template <typename Algo>
hipError_t rocprim_run(DevBuf &temp, Algo algo)
{
  size_t bytes = 0;
  hipError_t e = algo(nullptr, bytes);
  if (e == hipSuccess && temp.alloc(bytes) != 0)
  {
    e = hipErrorOutOfMemory;
  }
  return e == hipSuccess ? algo(temp.p, bytes) : e;
}

// offsets[] = exclusive sums of counts[0..n], whose last entry is 0;
// *total = offsets[n], i.e. the sum of all counts (search_common.hip)
VSA_HIDDEN int exclusive_sum(uint64_t *counts, uint64_t *offsets, uint64_t n,
                             hipStream_t stream, uint64_t *total);

inline uint64_t blocksfor(uint64_t items)
{
  return (items + VSA_BLOCK - 1) / VSA_BLOCK;
}

inline dim3 gridfor(uint64_t items)
{
  return vsa_grid(blocksfor(items));
}

struct KeepToU32
{
  __device__ uint32_t operator()(uint8_t k) const
  {
    return k;
  }
};

// out[] = the records of in[] with keep != 0, in order; *nkept (device) = count
VSA_HIDDEN int compact_matches(const vsa_match *in, const uint8_t *keep,
                               uint64_t count, vsa_match *out, uint64_t *nkept,
                               hipStream_t stream);

VSA_HIDDEN int sumlengths(const vsa_match *matches, uint64_t n,
                          hipStream_t stream, uint64_t *result);

// The end of a driver: the call is over when the stream is, and its n
// matches, the two times and the sum of the lengths go into the result.
inline int finish(vsa_result *res, DevBuf &matches, uint64_t n, Timer &tall,
                  Timer &tsearch, hipStream_t stream)
{
  tall.stop();
  VSA_HIP(hipStreamSynchronize(stream));
  res->count = n;
  res->matches = (vsa_match *) matches.release();
  res->stats.count = n;
  res->stats.search_kernel_ms = tsearch.ms();
  res->stats.total_device_ms = tall.ms();
  return sumlengths(res->matches, n, stream, &res->stats.sumlength);
}

inline unsigned int bitsfor(uint64_t maxvalue)
{
  unsigned int b = 1;
  while (b < 64 && (maxvalue >> b) != 0)
  {
    b++;
  }
  return b;
}

// out[t] = in[order[t]]
VSA_HIDDEN hipError_t gather_matches(const vsa_match *in,
                                     const uint32_t *order, uint64_t n,
                                     vsa_match *out, hipStream_t stream);

// stable sort of (key, match) pairs by key bits [0, endbit); results land in
// keys_out / matches_out.  The 32-byte records do not travel through the
// radix passes: (key, index) pairs do, and one gather follows.
VSA_HIDDEN int sortbykey(uint64_t *keys_in, uint64_t *keys_out, vsa_match *in,
                         vsa_match *out, uint64_t n, unsigned int endbit,
                         hipStream_t stream);

// stable sort of (key, index) pairs by key bits [0, endbit) (fewer than 2^32
// pairs)
VSA_HIDDEN int sortpairs(uint64_t *keys_in, uint64_t *keys_out,
                         uint32_t *vals_in, uint32_t *vals_out, uint64_t n,
                         unsigned int endbit, hipStream_t stream);

VSA_HIDDEN vsa_result *newresult(int device);

// owns a result until it is handed over (r = nullptr)
struct ResultGuard
{
  vsa_result *r;
  ~ResultGuard()
  {
    if (r != nullptr)
    {
      vsa_result_free(r);
    }
  }
};

// the first step of an entry point of a handle: its device, and the default
// stream for what it allocates
inline int enter(int device)
{
  if (vsa_set_device(device) != 0)
  {
    return -100;
  }
  vsa_dev_set_stream(nullptr);
  return 0;
}

// the query Multiseq of a view of select_rules.h: (*qstart)[] and (*qlen)[],
// nq words each in host memory (or null: none), go into device memory, which
// the handle owns through *d_qstart and *d_qlen; *qstart and *qlen then point
// there
inline int upload_queryview(uint64_t nq, const uint64_t **qstart,
                            const uint64_t **qlen, uint64_t **d_qstart,
                            uint64_t **d_qlen, const char *who)
{
  const size_t bytes = (size_t) nq * 8;
  if (*qstart != nullptr && bytes > 0 &&
      (vsa_hip_malloc((void **) d_qstart, bytes) != hipSuccess ||
       vsa_hip_malloc((void **) d_qlen, bytes) != hipSuccess ||
       hipMemcpy(*d_qstart, *qstart, bytes, hipMemcpyHostToDevice) !=
           hipSuccess ||
       hipMemcpy(*d_qlen, *qlen, bytes, hipMemcpyHostToDevice) != hipSuccess))
  {
    VSA_ERROR("%s: upload of the query Multiseq failed", who);
    return -100;
  }
  *qstart = *d_qstart;
  *qlen = *d_qlen;
  return 0;
}

// offsets[sh] = sum of the fill counts of the cursor regions before sh (one
// cursor per VSA_CURSOR_STRIDE words); summary = {total, largest count, 0, 0}
VSA_HIDDEN hipError_t shard_summary(const unsigned long long *cursors,
                                    uint32_t nshards, uint64_t *offsets,
                                    uint64_t *summary, hipStream_t stream);

struct U32ToU64
{
  __device__ uint64_t operator()(uint32_t v) const
  {
    return v;
  }
};

#endif
