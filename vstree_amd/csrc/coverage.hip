// Match coverage on the device: vmatch -dbnomatch / -qnomatch / -dbmaskmatch /
// -qmaskmatch (Vmatch/markmat.c, nomatch.c, showmasked.c, initpost.c:28-74,
// 156-267) on match lists that stay in HBM.
//
// The table is the reference's marktable with a layout of our own: one bit
// per position of a Multiseq, LSB first in 64-bit words (position p = bit
// p & 63 of word p >> 6), the bits behind the last position always 0.  Word
// index and bit arithmetic are 64 bit throughout: tables of 2^32 bits and
// more are addressed like the others.  The table is written with atomicOr and
// nothing else once it is initialised (no plain store meets an atomic).
//
//   mark     k_cov_mark: one record per lane, the one or two instances
//            markmatches selects.  An instance below VSA_COVERAGE_COOP_THRESHOLD
//            positions is set by its lane (a read of 100 symbols touches two
//            or three words); a longer one is handed to the whole wavefront,
//            lane l taking words l, l + 64, ... of it.  A word whose bits are
//            set already is not written again (read before atomic: repeat
//            lists put thousands of instances on the same words).
//   extract  the maximal runs of clear bits inside [first, first + len): per
//            word the run starts (clear, predecessor set or outside) and the
//            run ends; both go through the three steps of tile_compact.inc
//            -- count per tile, exclusive_sum() of the tile counts, write in
//            order -- in kernels of their own (k_cov_tilecount, k_cov_emit:
//            one word gives 0 to 64 positions, and the counts are 64 bit), so
//            the k-th start pairs with the k-th end; the runs of at least
//            minlength then go through the compaction of tile_compact.inc
//            itself (RunF), and get their sequence number from a binary
//            search in the separator positions.
//   count    popcount reduction; separators are set from the start, so marked
//            positions = set bits - separators.
//   merge    OR of one table into another.
#include "search_host.hpp"
#include "tile_compact.inc"

#define COV_TILE TC_TILE // words of the table per tile of the extraction

static_assert(COV_TILE * 64 == VSA_COVERAGE_EXTRACT_TILE,
              "the header names the tile of the extraction kernels");

struct vsa_coverage
{
  int device;
  int kind;       // 0: over an index, 1: over a query batch
  uint64_t nbits; // positions of the Multiseq
  uint64_t nwords;
  uint64_t *bits;   // device [nwords]
  uint64_t *seppos; // device [nsep], ascending
  uint64_t nsep;
  // over an index with queries: DATABASELENGTH and the number of database
  // sequences
  int hasindexedqueries;
  uint64_t dblength, numofdbsequences;
  // over a query batch
  uint64_t nq, seqoffset;
  uint32_t uniformlen; // != 0: every query has this length
  double mark_ms, extract_ms;
};

namespace
{

// ---- initialisation -------------------------------------------------------

// separator bits of a text: one word per wavefront step, the 64 lanes read
// 64 consecutive symbols
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_sepbits(const uint8_t *__restrict__ tis, uint64_t n,
              uint64_t *__restrict__ bits, uint64_t nwords)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t wavesperblock = TC_BLOCK / 64;
  uint64_t w = vsa_bid() * wavesperblock + (threadIdx.x >> 6);
  const uint64_t stride = vsa_nblocks() * wavesperblock;
  for (; w < nwords; w += stride)
  {
    const uint64_t p = w * 64 + lane;
    const bool sep = p < n && tis[p] == VSA_SEPARATOR;
    const uint64_t word = __ballot(sep);
    if (lane == 0)
    {
      bits[w] = word;
    }
  }
}

// separator positions of a batch of reads of one length m: (i + 1)(m + 1) - 1
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_uniform_seppos(uint64_t *__restrict__ seppos, uint64_t nsep, uint64_t m)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i < nsep)
  {
    seppos[i] = (i + 1) * (m + 1) - 1;
  }
}

// sets the bits at the given positions (the separators of a query table)
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_setbits(uint64_t *__restrict__ bits, uint64_t nbits,
              const uint64_t *__restrict__ pos, uint64_t npos)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i < npos && pos[i] < nbits)
  {
    atomicOr((unsigned long long *) &bits[pos[i] >> 6], 1ull << (pos[i] & 63));
  }
}

// ---- mark -----------------------------------------------------------------

struct CovMark
{
  uint64_t *bits;
  uint64_t nbits;
  const uint64_t *seppos;
  uint64_t nsep;
  int layout, markdb, palindromic;
  int markleft, markright, leftifdiff, rightifdiff;
  int readfirst;
  // index with queries (self layout)
  int hasindexedqueries;
  uint64_t dblength, numofdbsequences;
  // query table
  uint64_t nq, seqoffset;
  uint32_t uniformlen;
};

// number of separators in front of position p = its sequence number
__device__ __forceinline__ uint64_t cov_seqnum(const uint64_t *__restrict__ seppos,
                                               uint64_t nsep, uint64_t p)
{
  uint64_t lo = 0, hi = nsep;
  while (lo < hi)
  {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (seppos[mid] < p)
    {
      lo = mid + 1;
    }
    else
    {
      hi = mid;
    }
  }
  return lo;
}

__device__ __forceinline__ void cov_orword(uint64_t *bits, uint64_t w,
                                           uint64_t mask, int readfirst)
{
  if (readfirst && (bits[w] & mask) == mask)
  {
    return;
  }
  atomicOr((unsigned long long *) &bits[w], (unsigned long long) mask);
}

// bits [p, p + len) of word w (which the interval meets)
__device__ __forceinline__ uint64_t cov_wordmask(uint64_t w, uint64_t p,
                                                 uint64_t len)
{
  const uint64_t base = w << 6, end = p + len;
  uint64_t m = ~0ull;
  if (p > base)
  {
    m &= ~0ull << (p - base);
  }
  if (end < base + 64)
  {
    m &= ~(~0ull << (end - base));
  }
  return m;
}

// one instance [p, p + len), by one lane
__device__ __forceinline__ void cov_set_short(const CovMark &a, uint64_t p,
                                              uint64_t len)
{
  const uint64_t w1 = (p + len - 1) >> 6;
  for (uint64_t w = p >> 6; w <= w1; w++)
  {
    cov_orword(a.bits, w, cov_wordmask(w, p, len), a.readfirst);
  }
}

// the instances of the lanes of a wavefront: short ones lane by lane, long
// ones one after the other by all 64 lanes.  Every lane of the wavefront
// calls this (len = 0: nothing to set).
__device__ __forceinline__ void cov_set_instances(const CovMark &a, uint64_t p,
                                                  uint64_t len)
{
  // clamp to the table: nothing is ever written outside it
  if (p >= a.nbits)
  {
    len = 0;
  }
  else if (len > a.nbits - p)
  {
    len = a.nbits - p;
  }
  const bool islong = len >= VSA_COVERAGE_COOP_THRESHOLD;
  if (len > 0 && !islong)
  {
    cov_set_short(a, p, len);
  }
  uint64_t todo = __ballot(islong);
  const uint32_t lane = threadIdx.x & 63u;
  while (todo != 0)
  {
    const int src = __ffsll((unsigned long long) todo) - 1;
    todo &= todo - 1;
    const uint64_t lp = vsa_shfl64(p, src), ll = vsa_shfl64(len, src);
    const uint64_t w1 = (lp + ll - 1) >> 6;
    for (uint64_t w = (lp >> 6) + lane; w <= w1; w += 64)
    {
      cov_orword(a.bits, w, cov_wordmask(w, lp, ll), a.readfirst);
    }
  }
}

// markmatches (Vmatch/markmat.c:42-118) for one record per lane
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_mark(CovMark a, const vsa_match *__restrict__ matches, uint64_t count)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  // whole wavefronts behind the last record leave together
  if ((i & ~63ull) >= count)
  {
    return;
  }
  uint64_t p1 = 0, l1 = 0, p2 = 0, l2 = 0;
  if (i < count)
  {
    const vsa_match m = matches[i];
    if (a.layout == VSA_COVERAGE_SELF)
    {
      // Storeposition1/2, Storeseqnum1/2 of convertthematch
      // (Vmatch/procfinal.c:450-475): with queries inside the index the
      // second instance counts from the first query sequence
      uint64_t pos2 = m.queryseq;
      bool different = true;
      if (!(a.leftifdiff && a.rightifdiff))
      {
        const uint64_t s1 = cov_seqnum(a.seppos, a.nsep, m.dbstart);
        uint64_t s2 = cov_seqnum(a.seppos, a.nsep, m.queryseq);
        if (a.hasindexedqueries)
        {
          s2 -= a.numofdbsequences;
        }
        different = s1 != s2;
      }
      if (a.markdb)
      {
        if (a.markleft && (a.leftifdiff || different))
        {
          p1 = m.dbstart;
          l1 = m.length;
        }
        // hasnoqueryfiles: the right instance goes into the same table, at
        // Storeposition2 with offset 0 -- for an index with queries that is
        // the position counted from the first query sequence, as the
        // reference does it
        if (a.markright && (a.rightifdiff || different))
        {
          p2 = a.hasindexedqueries ? pos2 - a.dblength - 1 : pos2;
          l2 = m.length;
          if (a.hasindexedqueries && pos2 < a.dblength + 1)
          {
            l2 = 0;
          }
        }
      }
      else if (a.rightifdiff || different)
      {
        // offset DATABASELENGTH + 1 + Storeposition2 = the absolute position
        p2 = pos2;
        l2 = m.length;
      }
    }
    else if (a.markdb)
    {
      // query and approximate layout: the left instance only (-q)
      if (a.markleft)
      {
        p1 = m.dbstart;
        l1 = m.length;
      }
    }
    else
    {
      // the right instance in the table of the query Multiseq
      const uint64_t q = m.queryseq - a.seqoffset;
      if (m.queryseq >= a.seqoffset && q < a.nq)
      {
        uint64_t start, qlen;
        if (a.uniformlen != 0)
        {
          start = q * ((uint64_t) a.uniformlen + 1);
          qlen = a.uniformlen;
        }
        else
        {
          start = q == 0 ? 0 : a.seppos[q - 1] + 1;
          qlen = (q < a.nsep ? a.seppos[q] : a.nbits) - start;
        }
        uint64_t rel = m.querystart;
        bool ok = rel <= qlen && m.length <= qlen - rel;
        if (ok && a.palindromic)
        {
          // Vmatch/procfinal.c:152-158
          rel = qlen - (rel + m.length);
        }
        if (ok)
        {
          p2 = start + rel;
          l2 = m.length;
        }
      }
    }
  }
  cov_set_instances(a, p1, l1);
  cov_set_instances(a, p2, l2);
}

// ---- extract --------------------------------------------------------------

struct CovRange
{
  const uint64_t *bits;
  uint64_t nwords;
  uint64_t first, end; // positions [first, end)
  uint64_t w0, nw;     // words first >> 6 .. (end - 1) >> 6
};

// word w of the table with every position outside [first, end) taken as set
__device__ __forceinline__ uint64_t cov_eff(const CovRange &r, int64_t w)
{
  if (w < 0 || (uint64_t) w >= r.nwords)
  {
    return ~0ull;
  }
  const uint64_t base = (uint64_t) w << 6;
  if (base + 64 <= r.first || base >= r.end)
  {
    return ~0ull;
  }
  uint64_t v = r.bits[w];
  if (base < r.first)
  {
    v |= ~(~0ull << (r.first - base));
  }
  if (r.end < base + 64)
  {
    v |= ~0ull << (r.end - base);
  }
  return v;
}

// MODE 0: the word itself; 1: first positions of runs of clear bits; 2: last
// positions of such runs
template <int MODE>
__device__ __forceinline__ uint64_t cov_derived(const CovRange &r, uint64_t k)
{
  const int64_t w = (int64_t) (r.w0 + k);
  if (MODE == 0)
  {
    return r.bits[w];
  }
  const uint64_t v = cov_eff(r, w);
  if (v == ~0ull)
  {
    return 0;
  }
  if (MODE == 1)
  {
    return ~v & ((v << 1) | (cov_eff(r, w - 1) >> 63));
  }
  return ~v & ((v >> 1) | (cov_eff(r, w + 1) << 63));
}

template <int MODE>
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_tilecount(CovRange r, uint64_t *__restrict__ tilecount)
{
  const uint64_t tile = vsa_bid();
  if (tile * COV_TILE >= r.nw)
  {
    return;
  }
  __shared__ uint64_t sh[TC_BLOCK / 64];
  // thread t takes words t, t + TC_BLOCK, ... of the tile: coalesced, and the
  // order does not matter for a count
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
    const uint64_t k = tile * COV_TILE + (uint64_t) j * TC_BLOCK + threadIdx.x;
    if (k < r.nw)
    {
      c += (uint64_t) __popcll((unsigned long long) cov_derived<MODE>(r, k));
    }
  }
  uint64_t total;
  (void) vsa_block_exclusive_scan<0, TC_BLOCK>(c, sh, total);
  if (threadIdx.x == 0)
  {
    tilecount[tile] = total;
  }
}

// positions of the set bits of the derived words, ascending
template <int MODE>
__global__ void __launch_bounds__(TC_BLOCK)
k_cov_emit(CovRange r, const uint64_t *__restrict__ tileoffset,
           uint64_t *__restrict__ out, uint64_t capacity)
{
  const uint64_t tile = vsa_bid();
  if (tile * COV_TILE >= r.nw)
  {
    return;
  }
  __shared__ uint64_t sh[TC_BLOCK / 64];
  // thread t takes TC_IPT consecutive words: the positions come out in order
  const uint64_t k0 = tile * COV_TILE + (uint64_t) threadIdx.x * TC_IPT;
  uint64_t word[TC_IPT];
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
    word[j] = k0 + j < r.nw ? cov_derived<MODE>(r, k0 + j) : 0;
    c += (uint64_t) __popcll((unsigned long long) word[j]);
  }
  uint64_t total;
  uint64_t o = tileoffset[tile] +
               vsa_block_exclusive_scan<0, TC_BLOCK>(c, sh, total);
#pragma unroll
  for (int j = 0; j < TC_IPT; j++)
  {
    uint64_t v = word[j];
    while (v != 0)
    {
      const int b = __ffsll((unsigned long long) v) - 1;
      v &= v - 1;
      if (o < capacity)
      {
        out[o] = ((r.w0 + k0 + j) << 6) + (uint64_t) b;
      }
      o++;
    }
  }
}

// the runs [start[k], last[k]] of at least minlength positions, in order, as
// (length, absolute start, sequence number, relative start)
struct RunF
{
  typedef NoPayload Payload;
  const uint64_t *start, *last;
  uint64_t minlength;
  const uint64_t *seppos;
  uint64_t nsep;
  vsa_match *out;
  uint64_t capacity;

  __device__ int cls(uint64_t k, Payload &) const
  {
    return last[k] - start[k] + 1 >= minlength ? 0 : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t k, const Payload &) const
  {
    const uint64_t s = start[k];
    const uint64_t seq = cov_seqnum(seppos, nsep, s);
    if (rank < capacity)
    {
      vsa_match m;
      m.length = last[k] - s + 1;
      m.dbstart = s;
      m.queryseq = seq;
      m.querystart = s - (seq == 0 ? 0 : seppos[seq - 1] + 1);
      out[rank] = m;
    }
  }
};

// ---- count, merge ---------------------------------------------------------

__global__ void __launch_bounds__(TC_BLOCK)
k_cov_popcount(const uint64_t *__restrict__ bits, uint64_t nwords,
               unsigned long long *__restrict__ sum)
{
  __shared__ uint64_t sh[TC_BLOCK / 64];
  uint64_t c = 0;
  for (uint64_t w = vsa_bid() * TC_BLOCK + threadIdx.x; w < nwords;
       w += vsa_nblocks() * TC_BLOCK)
  {
    c += (uint64_t) __popcll((unsigned long long) bits[w]);
  }
  uint64_t total;
  (void) vsa_block_exclusive_scan<0, TC_BLOCK>(c, sh, total);
  if (threadIdx.x == 0 && total != 0)
  {
    atomicAdd(sum, (unsigned long long) total);
  }
}

__global__ void __launch_bounds__(TC_BLOCK)
k_cov_merge(uint64_t *__restrict__ dst, const uint64_t *__restrict__ src,
            uint64_t nwords)
{
  for (uint64_t w = vsa_bid() * TC_BLOCK + threadIdx.x; w < nwords;
       w += vsa_nblocks() * TC_BLOCK)
  {
    const uint64_t s = src[w];
    if ((dst[w] & s) != s)
    {
      atomicOr((unsigned long long *) &dst[w], (unsigned long long) s);
    }
  }
}

// ---- host -----------------------------------------------------------------

// the tile counts of the derived words of MODE scanned into offsets (nt + 1
// words); *total = their sum
template <int MODE>
int cov_count(const CovRange &r, uint64_t nt, DevBuf &offsets, uint64_t *total)
{
  DevBuf counts;
  if (counts.alloc((nt + 1) * 8) != 0 || offsets.alloc((nt + 1) * 8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(counts.as<uint64_t>() + nt, 0, 8, nullptr));
  k_cov_tilecount<MODE><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
      r, counts.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  return exclusive_sum(counts.as<uint64_t>(), offsets.as<uint64_t>(), nt,
                       nullptr, total);
}

int new_table(vsa_coverage *c)
{
  c->nwords = (c->nbits + 63) / 64;
  VSA_HIP(vsa_hip_malloc((void **) &c->bits, (c->nwords + 1) * 8));
  VSA_HIP(hipMemsetAsync(c->bits, 0, (c->nwords + 1) * 8, nullptr));
  return 0;
}

// positions of the set bits of the table (the separators, right after the
// table was made) into c->seppos
int collect_separators(vsa_coverage *c)
{
  c->nsep = 0;
  c->seppos = nullptr;
  if (c->nwords == 0)
  {
    return 0;
  }
  CovRange r = {c->bits, c->nwords, 0, c->nbits, 0, c->nwords};
  const uint64_t nt = tilesof(r.nw);
  DevBuf offsets;
  if (cov_count<0>(r, nt, offsets, &c->nsep) != 0)
  {
    return -100;
  }
  VSA_HIP(vsa_hip_malloc((void **) &c->seppos, (c->nsep + 1) * 8));
  if (c->nsep > 0)
  {
    k_cov_emit<0><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
        r, offsets.as<uint64_t>(), c->seppos, c->nsep);
    VSA_HIP(hipGetLastError());
  }
  VSA_HIP(hipStreamSynchronize(nullptr));
  return 0;
}

int readfirst_default()
{
  // VSA_COVERAGE_READFIRST=0: every word gets its atomic (the probe measures
  // both forms)
  const char *e = getenv("VSA_COVERAGE_READFIRST");
  return (e != nullptr && e[0] == '0') ? 0 : 1;
}

} // namespace

extern "C" uint64_t vsa_coverage_coop_threshold(void)
{
  return VSA_COVERAGE_COOP_THRESHOLD;
}

extern "C" void vsa_coverage_close(vsa_coverage *c)
{
  if (c == nullptr)
  {
    return;
  }
  (void) hipSetDevice(c->device);
  (void) hipFree(c->bits);
  (void) hipFree(c->seppos);
  delete c;
}

extern "C" int vsa_coverage_open_index(const vsa_index *index,
                                       vsa_coverage **coverage)
{
  if (index == nullptr || coverage == nullptr)
  {
    VSA_ERROR("vsa_coverage_open_index: NULL argument");
    return -1;
  }
  *coverage = nullptr;
  if (enter(index->device) != 0)
  {
    return -100;
  }
  vsa_coverage *c = new vsa_coverage();
  c->device = index->device;
  c->kind = 0;
  c->nbits = index->n;
  int rc = new_table(c);
  if (rc == 0 && c->nwords > 0)
  {
    k_cov_sepbits<<<stride_grid(c->nwords, 4096), TC_BLOCK, 0, nullptr>>>(
        index->tis_alloc + VSA_TIS_FRONTPAD, index->n, c->bits, c->nwords);
  }
  if (rc == 0)
  {
    rc = collect_separators(c);
  }
  if (rc == 0 && index->hasindexedqueries)
  {
    c->hasindexedqueries = 1;
    c->dblength = index->querysepposition;
    // sequences in front of the separator between database and queries
    uint64_t lo = 0;
    std::vector<uint64_t> sp(c->nsep);
    if (c->nsep > 0 &&
        hipMemcpy(sp.data(), c->seppos, c->nsep * 8, hipMemcpyDeviceToHost) !=
            hipSuccess)
    {
      VSA_ERROR("vsa_coverage_open_index: download of the separators failed");
      rc = -100;
    }
    lo = (uint64_t) (std::lower_bound(sp.begin(), sp.end(), c->dblength) -
                     sp.begin());
    c->numofdbsequences = lo + 1;
  }
  if (rc != 0)
  {
    vsa_coverage_close(c);
    return rc;
  }
  *coverage = c;
  return 0;
}

extern "C" int vsa_coverage_open_queries(const vsa_queries *q,
                                         vsa_coverage **coverage)
{
  if (q == nullptr || coverage == nullptr)
  {
    VSA_ERROR("vsa_coverage_open_queries: NULL argument");
    return -1;
  }
  *coverage = nullptr;
  if (enter(q->device) != 0)
  {
    return -100;
  }
  vsa_coverage *c = new vsa_coverage();
  c->device = q->device;
  c->kind = 1;
  c->nq = q->nq;
  c->seqoffset = q->seqoffset;
  c->nsep = q->nq > 0 ? q->nq - 1 : 0;
  const bool uniform = q->uniform && q->maxlength < 0xFFFFFFFFull;
  c->uniformlen = uniform ? (uint32_t) q->maxlength : 0;
  std::vector<uint64_t> sp;
  if (q->nq == 0)
  {
    c->nbits = 0;
  }
  else if (uniform)
  {
    c->nbits = q->nq * q->maxlength + c->nsep;
  }
  else
  {
    // sequence i starts at the sum of (length_j + 1), j < i
    // (kurtz-basic/multiseq.c:129-166)
    sp.resize(c->nsep);
    uint64_t pos = 0;
    for (uint64_t i = 0; i < q->nq; i++)
    {
      pos += q->hlength[i];
      if (i + 1 < q->nq)
      {
        sp[i] = pos++;
      }
    }
    c->nbits = pos;
  }
  int rc = new_table(c);
  if (rc == 0 && vsa_hip_malloc((void **) &c->seppos, (c->nsep + 1) * 8) != hipSuccess)
  {
    VSA_ERROR("vsa_coverage_open_queries: out of device memory");
    rc = -100;
  }
  if (rc == 0 && c->nsep > 0)
  {
    if (uniform)
    {
      k_cov_uniform_seppos<<<gridfor(c->nsep),
                             TC_BLOCK, 0, nullptr>>>(c->seppos, c->nsep,
                                                      q->maxlength);
    }
    else if (hipMemcpy(c->seppos, sp.data(), c->nsep * 8,
                       hipMemcpyHostToDevice) != hipSuccess)
    {
      VSA_ERROR("vsa_coverage_open_queries: upload of the separators failed");
      rc = -100;
    }
    if (rc == 0)
    {
      k_cov_setbits<<<gridfor(c->nsep),
                      TC_BLOCK, 0, nullptr>>>(c->bits, c->nbits, c->seppos,
                                               c->nsep);
    }
  }
  if (rc == 0 && hipStreamSynchronize(nullptr) != hipSuccess)
  {
    VSA_ERROR("vsa_coverage_open_queries: device error");
    rc = -100;
  }
  if (rc != 0)
  {
    vsa_coverage_close(c);
    return rc;
  }
  *coverage = c;
  return 0;
}

extern "C" int vsa_coverage_mark(vsa_coverage *c, const vsa_result *r,
                                 const vsa_coverageparams *p)
{
  if (c == nullptr || r == nullptr || p == nullptr)
  {
    VSA_ERROR("vsa_coverage_mark: NULL argument");
    return -1;
  }
  if (r->packbits != 0)
  {
    VSA_ERROR("vsa_coverage_mark: a packed candidate result has no records "
              "to mark");
    return VSA_NOT_COVERED;
  }
  if (r->extended)
  {
    VSA_ERROR("vsa_coverage_mark: lists of extended seeds "
              "(VSA_SINK_QUERY_HAMMING, VSA_SINK_SELF_HAMMING, "
              "VSA_SINK_QUERY_EDIST, VSA_SINK_SELF_EDIST) are not covered");
    return VSA_NOT_COVERED;
  }
  if (p->selfpalindromic)
  {
    VSA_ERROR("vsa_coverage_mark: lists of vmatch -p IDX (selfpalindromic) "
              "are not covered");
    return VSA_NOT_COVERED;
  }
  const bool markdb = p->side == VSA_COVERAGE_DATABASE;
  if (p->layout != VSA_COVERAGE_QUERY && p->layout != VSA_COVERAGE_SELF &&
      p->layout != VSA_COVERAGE_APPROX)
  {
    VSA_ERROR("vsa_coverage_mark: illegal layout %d", p->layout);
    return -2;
  }
  if (!markdb && p->side != VSA_COVERAGE_QUERIES)
  {
    VSA_ERROR("vsa_coverage_mark: illegal side %d", p->side);
    return -2;
  }
  if (!markdb && (p->layout == VSA_COVERAGE_APPROX || p->complete))
  {
    // the reference marks query offsets in a table of the database
    // (Vmatch/initpost.c:25-26,66-70)
    VSA_ERROR("vsa_coverage_mark: the query side of -complete lists is not "
              "covered");
    return VSA_NOT_COVERED;
  }
  if (r->device != c->device)
  {
    VSA_ERROR("vsa_coverage_mark: result on device %d, table on device %d",
              r->device, c->device);
    return -2;
  }
  if (p->layout == VSA_COVERAGE_SELF)
  {
    if (c->kind != 0)
    {
      VSA_ERROR("vsa_coverage_mark: self matches need a table over the index");
      return -2;
    }
    if (!markdb && !c->hasindexedqueries)
    {
      // Vmatch/initpost.c:48-62
      VSA_ERROR("option -qnomatch requires index containing query sequences "
                "or option -q");
      return -2;
    }
    if (p->palindromic)
    {
      VSA_ERROR("vsa_coverage_mark: palindromic self matches are the "
                "selfpalindromic form");
      return VSA_NOT_COVERED;
    }
  }
  else
  {
    if ((markdb && c->kind != 0) || (!markdb && c->kind != 1))
    {
      VSA_ERROR("vsa_coverage_mark: the %s side needs a table over the %s",
                markdb ? "database" : "query", markdb ? "index" : "queries");
      return -2;
    }
    if (!p->markleftifdifferentsequence || !p->markrightifdifferentsequence)
    {
      // Vmatch/parsevm.c:70-80 (CHECKKEEPARG)
      VSA_ERROR("argument \"%s\" to option %s not allowed if option -q is "
                "used",
                !p->markleftifdifferentsequence ? "keepleftifsamesequence"
                                                : "keeprightifsamesequence",
                "-dbnomatch");
      return -2;
    }
  }
  if (vsa_set_device(c->device) != 0)
  {
    return -100;
  }
  c->mark_ms = 0;
  if (r->count == 0 || c->nbits == 0)
  {
    return 0;
  }
  CovMark a;
  a.bits = c->bits;
  a.nbits = c->nbits;
  a.seppos = c->seppos;
  a.nsep = c->nsep;
  a.layout = p->layout;
  a.markdb = markdb ? 1 : 0;
  a.palindromic = p->palindromic;
  a.markleft = p->markleft;
  a.markright = p->markright;
  a.leftifdiff = p->markleftifdifferentsequence;
  a.rightifdiff = p->markrightifdifferentsequence;
  a.readfirst = readfirst_default();
  a.hasindexedqueries = c->hasindexedqueries;
  a.dblength = c->dblength;
  a.numofdbsequences = c->numofdbsequences;
  a.nq = c->nq;
  a.seqoffset = c->seqoffset;
  a.uniformlen = c->uniformlen;
  Timer t(nullptr);
  t.start();
  k_cov_mark<<<gridfor(r->count), TC_BLOCK, 0, nullptr>>>(a, r->matches,
                                                          r->count);
  VSA_HIP(hipGetLastError());
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->mark_ms = t.ms();
  return 0;
}

extern "C" int vsa_coverage_merge(vsa_coverage *dst, const vsa_coverage *src)
{
  if (dst == nullptr || src == nullptr)
  {
    VSA_ERROR("vsa_coverage_merge: NULL argument");
    return -1;
  }
  if (dst->nbits != src->nbits || dst->device != src->device)
  {
    VSA_ERROR("vsa_coverage_merge: tables of %lu and %lu positions on devices "
              "%d and %d",
              (unsigned long) dst->nbits, (unsigned long) src->nbits,
              dst->device, src->device);
    return -2;
  }
  if (vsa_set_device(dst->device) != 0)
  {
    return -100;
  }
  if (dst->nwords > 0 && dst != src)
  {
    k_cov_merge<<<stride_grid(dst->nwords, 4096), TC_BLOCK, 0, nullptr>>>(
        dst->bits, src->bits, dst->nwords);
    VSA_HIP(hipStreamSynchronize(nullptr));
  }
  return 0;
}

extern "C" int vsa_coverage_getstats(const vsa_coverage *c,
                                     vsa_coveragestats *stats)
{
  if (c == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_coverage_getstats: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  memset(stats, 0, sizeof *stats);
  stats->positions = c->nbits - c->nsep;
  stats->separators = c->nsep;
  stats->mark_ms = c->mark_ms;
  stats->extract_ms = c->extract_ms;
  if (c->nwords > 0)
  {
    DevBuf sum;
    if (sum.alloc(8) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(sum.p, 0, 8, nullptr));
    Timer t(nullptr);
    t.start();
    k_cov_popcount<<<stride_grid(c->nwords, 4096), TC_BLOCK, 0, nullptr>>>(
        c->bits, c->nwords, sum.as<unsigned long long>());
    t.stop();
    uint64_t set = 0;
    VSA_HIP(hipMemcpy(&set, sum.p, 8, hipMemcpyDeviceToHost));
    stats->count_ms = t.ms();
    // the separators are set from the start and stay set
    stats->marked = set - c->nsep;
  }
  return 0;
}

extern "C" uint64_t vsa_coverage_numofbits(const vsa_coverage *c)
{
  return c == nullptr ? 0 : c->nbits;
}

extern "C" int vsa_coverage_fetch_bits(const vsa_coverage *c, uint64_t *words,
                                       uint64_t capacity)
{
  if (c == nullptr || (words == nullptr && capacity > 0))
  {
    VSA_ERROR("vsa_coverage_fetch_bits: NULL argument");
    return -1;
  }
  const uint64_t m = std::min(capacity, c->nwords);
  if (m == 0)
  {
    return 0;
  }
  if (vsa_set_device(c->device) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemcpy(words, c->bits, m * 8, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" const void *vsa_coverage_device_bits(const vsa_coverage *c)
{
  return c == nullptr ? nullptr : c->bits;
}

static int cov_nomatch(vsa_coverage *c, uint64_t minlength, uint64_t first,
                       uint64_t len, vsa_result **intervals);

extern "C" int vsa_coverage_nomatch(vsa_coverage *c, uint64_t minlength,
                                    uint64_t first, uint64_t len,
                                    vsa_result **intervals)
{
  if (c == nullptr || intervals == nullptr)
  {
    VSA_ERROR("vsa_coverage_nomatch: NULL argument");
    return -1;
  }
  *intervals = nullptr;
  const int rc = cov_nomatch(c, minlength, first, len, intervals);
  if (rc != 0 && *intervals != nullptr)
  {
    vsa_result_free(*intervals);
    *intervals = nullptr;
  }
  return rc;
}

static int cov_nomatch(vsa_coverage *c, uint64_t minlength, uint64_t first,
                       uint64_t len, vsa_result **intervals)
{
  if (minlength < 1)
  {
    VSA_ERROR("vsa_coverage_nomatch: minlength must be >= 1");
    return -2;
  }
  if (first > c->nbits || len > c->nbits - first)
  {
    VSA_ERROR("vsa_coverage_nomatch: range [%lu, +%lu) lies outside the table "
              "of %lu positions",
              (unsigned long) first, (unsigned long) len,
              (unsigned long) c->nbits);
    return -2;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  vsa_result *res = newresult(c->device);
  *intervals = res;
  c->extract_ms = 0;
  if (len == 0)
  {
    return 0;
  }
  CovRange r;
  r.bits = c->bits;
  r.nwords = c->nwords;
  r.first = first;
  r.end = first + len;
  r.w0 = first >> 6;
  r.nw = ((r.end - 1) >> 6) - r.w0 + 1;
  const uint64_t nt = tilesof(r.nw);
  DevBuf ostart, olast, starts, lasts, offsets;
  uint64_t nruns = 0, nlast = 0, nout = 0;
  Timer t(nullptr);
  t.start();
  if (cov_count<1>(r, nt, ostart, &nruns) != 0 ||
      cov_count<2>(r, nt, olast, &nlast) != 0)
  {
    return -100;
  }
  if (nruns != nlast)
  {
    VSA_ERROR("vsa_coverage_nomatch: %lu run starts, %lu run ends",
              (unsigned long) nruns, (unsigned long) nlast);
    return -101;
  }
  if (nruns > 0)
  {
    if (starts.alloc(nruns * 8) != 0 || lasts.alloc(nruns * 8) != 0)
    {
      return -100;
    }
    k_cov_emit<1><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
        r, ostart.as<uint64_t>(), starts.as<uint64_t>(), nruns);
    k_cov_emit<2><<<vsa_grid(nt), TC_BLOCK, 0, nullptr>>>(
        r, olast.as<uint64_t>(), lasts.as<uint64_t>(), nruns);
    VSA_HIP(hipGetLastError());
    RunF rf = {starts.as<uint64_t>(), lasts.as<uint64_t>(), minlength,
               c->seppos, c->nsep, nullptr, 0};
    if (tc_count<1, 1>(rf, nruns, offsets, &nout) != 0)
    {
      return -100;
    }
    if (nout > 0)
    {
      if (vsa_dev_alloc((void **) &res->matches, nout * sizeof(vsa_match)) != 0)
      {
        return -100;
      }
      rf.out = res->matches;
      rf.capacity = nout;
      if (tc_emit<1>(rf, nruns, offsets) != 0)
      {
        return -100;
      }
    }
  }
  t.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  c->extract_ms = t.ms();
  res->count = nout;
  res->stats.count = nout;
  res->stats.total_device_ms = c->extract_ms;
  return 0;
}

extern "C" int vsa_coverage_nomatch_all(vsa_coverage *c, uint64_t minlength,
                                        vsa_result **intervals)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_coverage_nomatch_all: NULL argument");
    return -1;
  }
  return vsa_coverage_nomatch(c, minlength, 0, c->nbits, intervals);
}

extern "C" int vsa_coverage_nomatch_database(vsa_coverage *c,
                                             uint64_t minlength,
                                             vsa_result **intervals)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_coverage_nomatch_database: NULL argument");
    return -1;
  }
  // Vmatch/initpost.c:167-175: len = DATABASELENGTH = totallength -
  // totalquerylength - 1 (include/multidef.h:91): without queries in the index
  // the reference leaves the last position of the text out
  uint64_t len = c->nbits;
  if (c->kind == 0)
  {
    len = c->hasindexedqueries ? c->dblength : (c->nbits > 0 ? c->nbits - 1 : 0);
  }
  return vsa_coverage_nomatch(c, minlength, 0, len, intervals);
}

extern "C" int vsa_coverage_nomatch_queries(vsa_coverage *c,
                                            uint64_t minlength,
                                            vsa_result **intervals)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_coverage_nomatch_queries: NULL argument");
    return -1;
  }
  if (c->kind == 1)
  {
    return vsa_coverage_nomatch(c, minlength, 0, c->nbits, intervals);
  }
  if (!c->hasindexedqueries)
  {
    VSA_ERROR("option -qnomatch requires index containing query sequences "
              "or option -q");
    return -2;
  }
  // Vmatch/initpost.c:176-181: posoffset = DATABASELENGTH + 1, len =
  // totalquerylength
  return vsa_coverage_nomatch(c, minlength, c->dblength + 1,
                              c->nbits - c->dblength - 1, intervals);
}

// a match list the caller holds in host memory (fetched earlier, filtered or
// made by hand) as a result on the device
extern "C" int vsa_result_from_host(const vsa_match *matches, uint64_t count,
                                    int device, vsa_result **result)
{
  if (result == nullptr || (matches == nullptr && count > 0))
  {
    VSA_ERROR("vsa_result_from_host: NULL argument");
    return -1;
  }
  *result = nullptr;
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_result *r = newresult(device);
  r->count = count;
  r->stats.count = count;
  if (count > 0)
  {
    if (vsa_dev_alloc((void **) &r->matches, count * sizeof(vsa_match)) != 0)
    {
      delete r;
      return -100;
    }
    if (hipMemcpy(r->matches, matches, count * sizeof(vsa_match),
                  hipMemcpyHostToDevice) != hipSuccess)
    {
      VSA_ERROR("vsa_result_from_host: upload failed");
      vsa_result_free(r);
      return -100;
    }
    for (uint64_t i = 0; i < count; i++)
    {
      r->stats.sumlength += matches[i].length;
    }
  }
  *result = r;
  return 0;
}
