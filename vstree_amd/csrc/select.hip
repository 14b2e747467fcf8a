// Match selection on the device: vmatch -best N, -sort mode, -evalue,
// -identity, -leastscore and the gap bounds of -l L lo [hi]
// (Vmatch/procfinal.c:566-636,695-745, Vmatch/mokay.c, kurtz/bestmatch.c:
// 33-119) on match lists that stay in HBM.  The rules themselves -- what
// processfinal derives from a record, matchokay, the five key words of
// cmpBestMatch -- are select_rules.h, the same text the host compiles.
//
//   key      one lane per record: the record, the length and Multiseq start
//            of its query sequence, T with its line starts and hequot (made
//            by the host, select_host.c) -> E-value, matchokay, key.  The
//            survivors go through the stable compaction of
//            tile_compact.inc.  Filters only (N = 0): the records
//            themselves are appended to the list.  -best: the five
//            key words go into a pool, word by word (structure of arrays),
//            behind the keys of the selection so far.
//   select   the N-th smallest key of the pool by an MSD radix select, word
//            by word, 11 bits at a time: every workgroup counts the digits of
//            the candidates -- the keys equal to the threshold prefix found
//            so far -- in LDS and adds its counts to one table, the host
//            picks the digit.  Each pass also ANDs and ORs the candidates'
//            word: the bits all candidates share are skipped, so a word on
//            which they are all equal costs ONE pass, however many there are
//            (millions of full-length matches of equal-length reads tie on
//            E-value and length).  Then one three-class compaction
//            against the threshold: smaller keys are selected, of the equal
//            ones the first (they are one match), larger ones wait.
//   sort     the at most N selected keys: five stable rocPRIM radix sorts of
//            (word, index) pairs, last word first; equal neighbours are one
//            match.  Where duplicates left fewer than N distinct keys, the
//            waiting ones go through select again.
//   When the selection is full, its worst key is part of the rules of the
//   next vsa_select_add: a key that is not smaller never enters the pool.
// Positions, lengths and every index into a list are 64 bit; only the
// indices inside the selection (at most N < 2^32) are 32 bit.
#include "resident_list.hpp"
#include "select_internal.h"
#include "tile_compact.inc"

#define SEL_DIGITBITS 11
#define SEL_BINS (1 << SEL_DIGITBITS)
#define SEL_W VSA_SELECT_KEYWORDS

struct vsa_select
{
  int device = 0;
  int selfpalindromic = 0; // the layout says vmatch -p IDX: not covered
  vsa_selctx ctx;
  vsa_selrules drules; // ctx.rules with the pointers into device memory
  DeviceLayout layout;
  double *d_table = nullptr, *d_hequot = nullptr;
  int64_t *d_linestart = nullptr;
  // -best: the selection, sorted, distinct: key word w of entry j at
  // skeys[w * nsel + j]
  uint64_t nsel = 0;
  uint64_t *skeys = nullptr;
  vsa_match *srecs = nullptr;
  uint64_t worst[SEL_W];
  // filters only: the list so far
  ResidentList list;
  std::vector<uint8_t> lastflags; // of the list finish delivered last
  uint64_t lastpasses = 0;        // histogram kernels of the last add
  vsa_selectstats stats;
};

namespace
{

struct KeyPayload
{
  uint64_t key[SEL_W];
};

// a record through processfinal's arithmetic and matchokay.  Classes: 0 it
// goes on, 1 it does not fit the layout, 2 matchokay drops it, 3 it equals
// the worst key of a full selection (a duplicate); -1 it is worse than that.
struct KeyF
{
  typedef KeyPayload Payload;
  vsa_selrules r;
  const vsa_match *matches;
  int palindromic;
  // -best: the pool (key word w of entry j at keys[w * stride + j]) and the
  // record each entry came from
  uint64_t *keys;
  uint64_t stride, base;
  uint64_t *src;
  // filters only: the list
  vsa_match *lrecs;
  uint8_t *lflags;

  __device__ int cls(uint64_t i, Payload &p) const
  {
    const vsa_match m = matches[i];
    vsa_selvalues v;
    if (vsa_sel_values(&r, &m, palindromic, &v) != 0)
    {
      return 1;
    }
    if (!vsa_sel_okay(&r, &v))
    {
      return 2;
    }
    vsa_sel_key(&v, palindromic, p.key);
    if (r.hasworst)
    {
      const int c = vsa_sel_keycmp(p.key, r.worst);
      if (c >= 0)
      {
        return c == 0 ? 3 : -1;
      }
    }
    return 0;
  }
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &p) const
  {
    if (keys != nullptr)
    {
#pragma unroll
      for (int w = 0; w < SEL_W; w++)
      {
        keys[(uint64_t) w * stride + base + rank] = p.key[w];
      }
      src[rank] = i;
    }
    else
    {
      lrecs[base + rank] = matches[i];
      lflags[base + rank] = (uint8_t) (palindromic != 0);
    }
  }
};

// entries of the pool (those of `list`, or all) against the threshold:
// 0 smaller, 1 equal, 2 larger
struct ClassifyF
{
  typedef NoPayload Payload;
  const uint64_t *keys;
  uint64_t stride;
  const uint64_t *list;
  uint64_t T[SEL_W];
  uint64_t *selected; // smaller ones from selected[0], then ONE equal one
  uint64_t nless;
  uint64_t *waiting;

  __device__ uint64_t entry(uint64_t i) const
  {
    return list != nullptr ? list[i] : i;
  }
  __device__ int cls(uint64_t i, Payload &) const
  {
    const uint64_t e = entry(i);
#pragma unroll
    for (int w = 0; w < SEL_W; w++)
    {
      const uint64_t x = keys[(uint64_t) w * stride + e];
      if (x != T[w])
      {
        return x < T[w] ? 0 : 2;
      }
    }
    return 1;
  }
  __device__ void put(int q, uint64_t rank, uint64_t i, const Payload &) const
  {
    const uint64_t e = entry(i);
    if (q == 0)
    {
      selected[rank] = e;
    }
    else if (q == 2)
    {
      waiting[rank] = e;
    }
    else if (rank == 0)
    {
      selected[nless] = e;
    }
  }
};

// the sorted selection: 0 the first of a run of equal keys, 1 a duplicate
struct UniqueF
{
  typedef NoPayload Payload;
  const uint64_t *keys;
  uint64_t stride;
  const uint64_t *selected;
  const uint32_t *perm;
  uint64_t *out;

  __device__ int cls(uint64_t j, Payload &) const
  {
    if (j == 0)
    {
      return 0;
    }
    const uint64_t a = selected[perm[j - 1]], b = selected[perm[j]];
#pragma unroll
    for (int w = 0; w < SEL_W; w++)
    {
      if (keys[(uint64_t) w * stride + a] != keys[(uint64_t) w * stride + b])
      {
        return 0;
      }
    }
    return 1;
  }
  __device__ void put(int, uint64_t rank, uint64_t j, const Payload &) const
  {
    out[rank] = selected[perm[j]];
  }
};

// ---- the digit histogram of the radix select -------------------------------

struct HistArgs
{
  const uint64_t *keys;
  uint64_t stride;
  const uint64_t *list; // or nullptr: all n entries of the pool
  uint64_t n;
  int word;          // the word the select works on
  uint64_t T[SEL_W]; // the words before it
  uint64_t mask, value; // the bits of this word found so far
  int shift;
  uint32_t digitmask;
};

// hist[SEL_BINS] += digits of the candidates; andor[0] &= / andor[1] |= their
// word.  The counts of a workgroup are gathered in LDS; a wavefront whose
// candidates all show the same digit (the tie groups) adds once.
__global__ void __launch_bounds__(TC_BLOCK)
k_sel_hist(HistArgs a, unsigned long long *__restrict__ hist,
           unsigned long long *__restrict__ andor)
{
  __shared__ uint32_t lh[SEL_BINS];
  for (uint32_t b = threadIdx.x; b < SEL_BINS; b += TC_BLOCK)
  {
    lh[b] = 0;
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t wand = ~0ull, wor = 0;
  const uint64_t stride = vsa_nblocks() * TC_BLOCK;
  // whole wavefronts run the same number of rounds
  const uint64_t rounds = (a.n + stride - 1) / stride;
  uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  for (uint64_t r = 0; r < rounds; r++, i += stride)
  {
    bool cand = i < a.n;
    uint64_t x = 0;
    if (cand)
    {
      const uint64_t e = a.list != nullptr ? a.list[i] : i;
      for (int w = 0; cand && w < a.word; w++)
      {
        cand = a.keys[(uint64_t) w * a.stride + e] == a.T[w];
      }
      if (cand)
      {
        x = a.keys[(uint64_t) a.word * a.stride + e];
        cand = (x & a.mask) == a.value;
      }
    }
    const uint32_t digit = (uint32_t) (x >> a.shift) & a.digitmask;
    const uint64_t act = __ballot(cand);
    if (act != 0)
    {
      const int first = __ffsll((unsigned long long) act) - 1;
      const uint32_t d0 = __shfl(digit, first);
      const uint64_t same = __ballot(cand && digit == d0);
      if (same == act)
      {
        if (lane == (uint32_t) first)
        {
          atomicAdd(&lh[d0], (uint32_t) __popcll((unsigned long long) act));
        }
      }
      else if (cand)
      {
        atomicAdd(&lh[digit], 1u);
      }
    }
    if (cand)
    {
      wand &= x;
      wor |= x;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const uint32_t alo = __shfl_xor((uint32_t) wand, d);
    const uint32_t ahi = __shfl_xor((uint32_t) (wand >> 32), d);
    const uint32_t olo = __shfl_xor((uint32_t) wor, d);
    const uint32_t ohi = __shfl_xor((uint32_t) (wor >> 32), d);
    wand &= ((uint64_t) ahi << 32) | alo;
    wor |= ((uint64_t) ohi << 32) | olo;
  }
  // (a wavefront without a candidate still holds the neutral elements)
  if (lane == 0 && !(wand == ~0ull && wor == 0))
  {
    atomicAnd(&andor[0], (unsigned long long) wand);
    atomicOr(&andor[1], (unsigned long long) wor);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < SEL_BINS; b += TC_BLOCK)
  {
    if (lh[b] != 0)
    {
      atomicAdd(&hist[b], (unsigned long long) lh[b]);
    }
  }
}

// ---- small kernels -----------------------------------------------------------

// out[j] = word of the selected entry perm[j]
__global__ void __launch_bounds__(TC_BLOCK)
k_sel_gatherword(const uint64_t *__restrict__ word,
                 const uint64_t *__restrict__ selected,
                 const uint32_t *__restrict__ perm, uint64_t n,
                 uint64_t *__restrict__ out)
{
  const uint64_t j = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (j < n)
  {
    out[j] = word[selected[perm[j]]];
  }
}

// the new selection from the pool: entry e < nold is entry e of the old
// selection, another one the record src[e - nold] of the list
__global__ void __launch_bounds__(TC_BLOCK)
k_sel_commit(const uint64_t *__restrict__ keys, uint64_t stride,
             const uint64_t *__restrict__ selected, uint64_t n,
             const vsa_match *__restrict__ oldrecs, uint64_t nold,
             const vsa_match *__restrict__ matches,
             const uint64_t *__restrict__ src, uint64_t *__restrict__ newkeys,
             vsa_match *__restrict__ newrecs)
{
  const uint64_t j = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (j < n)
  {
    const uint64_t e = selected[j];
#pragma unroll
    for (int w = 0; w < SEL_W; w++)
    {
      newkeys[(uint64_t) w * n + j] = keys[(uint64_t) w * stride + e];
    }
    newrecs[j] = e < nold ? oldrecs[e] : matches[src[e - nold]];
  }
}

__global__ void __launch_bounds__(TC_BLOCK)
k_sel_flags(const uint64_t *__restrict__ word4, uint64_t n,
            uint8_t *__restrict__ flags)
{
  const uint64_t j = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (j < n)
  {
    flags[j] = (uint8_t) (word4[j] & 1u);
  }
}

// the largest querystart field (the distance of approximate matches)
__global__ void __launch_bounds__(TC_BLOCK)
k_sel_maxdistance(const vsa_match *__restrict__ matches, uint64_t n,
                  unsigned long long *__restrict__ out)
{
  uint64_t mx = 0;
  for (uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x; i < n;
       i += vsa_nblocks() * TC_BLOCK)
  {
    const uint64_t d = matches[i].querystart;
    mx = d > mx ? d : mx;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const uint32_t lo = __shfl_xor((uint32_t) mx, d);
    const uint32_t hi = __shfl_xor((uint32_t) (mx >> 32), d);
    const uint64_t o = ((uint64_t) hi << 32) | lo;
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63u) == 0 && mx != 0)
  {
    atomicMax(out, (unsigned long long) mx);
  }
}

__global__ void __launch_bounds__(TC_BLOCK)
k_sel_evalues(vsa_selrules r, const vsa_match *__restrict__ matches,
              uint64_t n, int palindromic, double *__restrict__ out,
              unsigned long long *__restrict__ bad)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i < n)
  {
    const vsa_match m = matches[i];
    vsa_selvalues v;
    if (vsa_sel_values(&r, &m, palindromic, &v) != 0)
    {
      v.evalue = 0.0;
      atomicAdd(bad, 1ull);
    }
    out[i] = v.evalue;
  }
}

// ---- host ----------------------------------------------------------------------

void free_tables(vsa_select *s)
{
  (void) hipFree(s->d_table);
  (void) hipFree(s->d_linestart);
  (void) hipFree(s->d_hequot);
  s->d_table = s->d_hequot = nullptr;
  s->d_linestart = nullptr;
}

// T, its line starts and hequot as the host made them, into device memory
int upload_tables(vsa_select *s)
{
  const vsa_selrules &h = s->ctx.rules;
  const size_t ntab = (size_t) s->ctx.ev.nexttab;
  free_tables(s);
  VSA_HIP(vsa_hip_malloc((void **) &s->d_table, (ntab + 1) * 8));
  VSA_HIP(vsa_hip_malloc((void **) &s->d_linestart, (h.nlines + 1) * 8));
  VSA_HIP(vsa_hip_malloc((void **) &s->d_hequot, h.nlines * 8));
  if (ntab > 0)
  {
    VSA_HIP(hipMemcpy(s->d_table, h.table, ntab * 8, hipMemcpyHostToDevice));
  }
  VSA_HIP(hipMemcpy(s->d_linestart, h.linestart, (h.nlines + 1) * 8,
                    hipMemcpyHostToDevice));
  VSA_HIP(hipMemcpy(s->d_hequot, h.hequot, h.nlines * 8,
                    hipMemcpyHostToDevice));
  s->drules = h;
  s->drules.table = s->d_table;
  s->drules.linestart = s->d_linestart;
  s->drules.hequot = s->d_hequot;
  s->drules.qstart = s->layout.d_qstart;
  s->drules.qlen = s->layout.d_qlen;
  return 0;
}

// the table reaches the largest distance of the list
int ensure_tables(vsa_select *s, const vsa_result *r)
{
  const int kind = s->ctx.rules.kind;
  if ((kind != VSA_SINK_APPROX_EDIST && kind != VSA_SINK_APPROX_HAMMING) ||
      r->count == 0)
  {
    return 0;
  }
  DevBuf mx;
  uint64_t maxd = 0;
  if (mx.alloc(8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(mx.p, 0, 8, nullptr));
  k_sel_maxdistance<<<stride_grid(r->count, 2048), TC_BLOCK, 0, nullptr>>>(
      r->matches, r->count, mx.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipMemcpy(&maxd, mx.p, 8, hipMemcpyDeviceToHost));
  const int grew = vsa_selctx_ensure(&s->ctx, maxd);
  if (grew < 0)
  {
    return grew;
  }
  return grew > 0 ? upload_tables(s) : 0;
}

// the gate of vsa_select_add and vsa_select_evalues
int check_list(const vsa_select *s, const vsa_result *r, int palindromic,
               const char *who)
{
  return gate(who, "select from", "selection", s, r,
              [&]() {
                return s->selfpalindromic
                           ? "lists of vmatch -p IDX (selfpalindromic) are "
                             "not covered"
                           : selfform(s->ctx.rules.kind, palindromic);
              },
              0, nullptr);
}

// The threshold of the radix select: T = the key of rank `need` (1 based,
// counted with duplicates) among the n entries of `list` (or of the whole
// pool).  Word by word; within a word the bits all candidates share cost
// nothing.  *passes counts the histogram kernels.
int sel_threshold(const uint64_t *keys, uint64_t stride, const uint64_t *list,
                  uint64_t n, uint64_t need, uint64_t *T, uint64_t *passes)
{
  DevBuf dev;
  std::vector<uint64_t> h(SEL_BINS + 2);
  if (dev.alloc((SEL_BINS + 2) * 8) != 0)
  {
    return -100;
  }
  HistArgs a;
  a.keys = keys;
  a.stride = stride;
  a.list = list;
  a.n = n;
  for (int w = 0; w < SEL_W; w++)
  {
    a.word = w;
    a.mask = a.value = 0;
    int top = 63;
    while (a.mask != ~0ull)
    {
      a.shift = top >= SEL_DIGITBITS - 1 ? top - (SEL_DIGITBITS - 1) : 0;
      a.digitmask = (uint32_t) ((1u << (top - a.shift + 1)) - 1u);
      h.assign(SEL_BINS + 2, 0);
      h[SEL_BINS] = ~0ull;
      VSA_HIP(hipMemcpyAsync(dev.p, h.data(), (SEL_BINS + 2) * 8,
                             hipMemcpyHostToDevice, nullptr));
      k_sel_hist<<<stride_grid(n, 2048), TC_BLOCK, 0, nullptr>>>(
          a, dev.as<unsigned long long>(),
          dev.as<unsigned long long>() + SEL_BINS);
      VSA_HIP(hipGetLastError());
      VSA_HIP(hipMemcpy(h.data(), dev.p, (SEL_BINS + 2) * 8,
                        hipMemcpyDeviceToHost));
      (*passes)++;
      uint64_t below = 0;
      uint32_t digit = 0;
      while (digit < SEL_BINS && below + h[digit] < need)
      {
        below += h[digit++];
      }
      if (digit == SEL_BINS)
      {
        VSA_ERROR("vsa_select: the digit counts of the select do not reach "
                  "rank %lu", (unsigned long) need);
        return -101;
      }
      need -= below;
      // the bits every candidate of this pass shares, then the digit
      const uint64_t common = ~(h[SEL_BINS] ^ h[SEL_BINS + 1]) & ~a.mask;
      a.value |= h[SEL_BINS] & common;
      a.mask |= common;
      const uint64_t window = (uint64_t) a.digitmask << a.shift;
      a.value = (a.value & ~window) | ((uint64_t) digit << a.shift);
      a.mask |= window;
      if (a.mask != ~0ull)
      {
        top = 63 - __builtin_clzll(~a.mask);
      }
    }
    a.T[w] = a.value;
    T[w] = a.value;
  }
  return 0;
}

// the n entries of `selected` in key order without duplicates -> out (room
// for n), *distinct = their number
int sel_sortunique(const uint64_t *keys, uint64_t stride,
                   const uint64_t *selected, uint64_t n, uint64_t *out,
                   uint64_t *distinct)
{
  DevBuf perm, perm2, kw, kw2, offsets;
  if (perm.alloc(n * 4) || perm2.alloc(n * 4) || kw.alloc(n * 8) ||
      kw2.alloc(n * 8))
  {
    return -100;
  }
  k_tc_iota<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(perm.as<uint32_t>(), n);
  VSA_HIP(hipGetLastError());
  uint32_t *p = perm.as<uint32_t>(), *p2 = perm2.as<uint32_t>();
  for (int w = SEL_W - 1; w >= 0; w--)
  {
    k_sel_gatherword<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
        keys + (uint64_t) w * stride, selected, p, n, kw.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    if (sortpairs(kw.as<uint64_t>(), kw2.as<uint64_t>(), p, p2, n, 64,
                  nullptr) != 0)
    {
      return -100;
    }
    std::swap(p, p2);
  }
  UniqueF u;
  u.keys = keys;
  u.stride = stride;
  u.selected = selected;
  u.perm = p;
  u.out = out;
  uint64_t totals[2];
  if (tc_count<1, 2>(u, n, offsets, totals) != 0 ||
      tc_emit<1>(u, n, offsets) != 0)
  {
    return -100;
  }
  VSA_HIP(hipStreamSynchronize(nullptr));
  *distinct = totals[0];
  return 0;
}

// -best: the pool of the old selection and the survivors of a list -> the new
// selection
int sel_best(vsa_select *s, const vsa_result *r, KeyF &kf, DevBuf &offsets,
             uint64_t m)
{
  const uint64_t N = s->ctx.params.bestnumber, nold = s->nsel, P = nold + m;
  DevBuf pool, src, sel, sel2, waiting;
  if (pool.alloc(SEL_W * P * 8) != 0 || src.alloc(m * 8) != 0)
  {
    return -100;
  }
  for (int w = 0; nold > 0 && w < SEL_W; w++)
  {
    VSA_HIP(hipMemcpyAsync(pool.as<uint64_t>() + (uint64_t) w * P,
                           s->skeys + (uint64_t) w * nold, nold * 8,
                           hipMemcpyDeviceToDevice, nullptr));
  }
  kf.keys = pool.as<uint64_t>();
  kf.stride = P;
  kf.base = nold;
  kf.src = src.as<uint64_t>();
  if (tc_emit<1>(kf, r->count, offsets) != 0)
  {
    return -100;
  }
  const uint64_t cap = std::min(P, N + 1);
  if (sel.alloc(cap * 8) != 0 || sel2.alloc(cap * 8) != 0)
  {
    return -100;
  }
  uint64_t nselected = 0, distinct = 0, duplicates = 0, passes = 0;
  const uint64_t *list = nullptr;
  uint64_t c = P;
  DevBuf listbuf;
  while (c > 0 && distinct < N)
  {
    const uint64_t k = N - distinct;
    if (c <= k)
    {
      // all of them
      if (list == nullptr)
      {
        k_tc_iota<<<gridfor(c), TC_BLOCK, 0, nullptr>>>(
            sel.as<uint64_t>() + nselected, c);
        VSA_HIP(hipGetLastError());
      }
      else
      {
        VSA_HIP(hipMemcpyAsync(sel.as<uint64_t>() + nselected, list, c * 8,
                               hipMemcpyDeviceToDevice, nullptr));
      }
      nselected += c;
      c = 0;
    }
    else
    {
      ClassifyF cf;
      cf.keys = pool.as<uint64_t>();
      cf.stride = P;
      cf.list = list;
      if (sel_threshold(cf.keys, P, list, c, k, cf.T, &passes) != 0)
      {
        return -100;
      }
      uint64_t totals[3];
      DevBuf coffsets, nextwaiting;
      cf.selected = nullptr;
      cf.waiting = nullptr;
      cf.nless = 0;
      if (tc_count<3, 3>(cf, c, coffsets, totals) != 0)
      {
        return -100;
      }
      if (totals[1] == 0 || totals[0] >= k)
      {
        VSA_ERROR("vsa_select: the threshold of rank %lu has %lu keys below "
                  "it and %lu equal ones", (unsigned long) k,
                  (unsigned long) totals[0], (unsigned long) totals[1]);
        return -101;
      }
      if (nextwaiting.alloc(totals[2] * 8) != 0)
      {
        return -100;
      }
      cf.selected = sel.as<uint64_t>() + nselected;
      cf.nless = totals[0];
      cf.waiting = nextwaiting.as<uint64_t>();
      if (tc_emit<3>(cf, c, coffsets) != 0)
      {
        return -100;
      }
      VSA_HIP(hipStreamSynchronize(nullptr));
      nselected += totals[0] + 1;
      duplicates += totals[1] - 1;
      c = totals[2];
      listbuf.free();
      listbuf.p = nextwaiting.release();
      list = listbuf.as<uint64_t>();
    }
    if (sel_sortunique(pool.as<uint64_t>(), P, sel.as<uint64_t>(), nselected,
                       sel2.as<uint64_t>(), &distinct) != 0)
    {
      return -100;
    }
    duplicates += nselected - distinct;
    nselected = distinct;
    std::swap(sel.p, sel2.p);
  }
  // the new selection
  DevBuf newkeys, newrecs;
  if (newkeys.alloc(SEL_W * distinct * 8) != 0 ||
      newrecs.alloc(distinct * sizeof(vsa_match)) != 0)
  {
    return -100;
  }
  if (distinct > 0)
  {
    k_sel_commit<<<gridfor(distinct), TC_BLOCK, 0, nullptr>>>(
        pool.as<uint64_t>(), P, sel.as<uint64_t>(), distinct, s->srecs, nold,
        r->matches, src.as<uint64_t>(), newkeys.as<uint64_t>(),
        newrecs.as<vsa_match>());
    VSA_HIP(hipGetLastError());
  }
  uint64_t worst[SEL_W];
  if (distinct == N)
  {
    for (int w = 0; w < SEL_W; w++)
    {
      VSA_HIP(hipMemcpyAsync(&worst[w],
                             newkeys.as<uint64_t>() + (uint64_t) w * distinct +
                                 (distinct - 1),
                             8, hipMemcpyDeviceToHost, nullptr));
    }
  }
  VSA_HIP(hipStreamSynchronize(nullptr));
  vsa_dev_free(s->skeys);
  vsa_dev_free(s->srecs);
  s->skeys = (uint64_t *) newkeys.release();
  s->srecs = (vsa_match *) newrecs.release();
  s->nsel = distinct;
  memcpy(s->worst, worst, sizeof worst);
  s->stats.duplicates += duplicates;
  s->lastpasses = passes;
  return 0;
}

} // namespace

extern "C" void vsa_select_close(vsa_select *s)
{
  if (s == nullptr)
  {
    return;
  }
  s->layout.release();
  free_tables(s);
  vsa_dev_free(s->skeys);
  vsa_dev_free(s->srecs);
  s->list.release();
  vsa_selctx_free(&s->ctx);
  delete s;
}

extern "C" int vsa_select_open(const vsa_sinkparams *layout,
                               const vsa_queries *queries,
                               const vsa_selectparams *params, int device,
                               vsa_select **select)
{
  if (layout == nullptr || params == nullptr || select == nullptr)
  {
    VSA_ERROR("vsa_select_open: NULL argument");
    return -1;
  }
  *select = nullptr;
  if (queries != nullptr && queries->device != device)
  {
    VSA_ERROR("vsa_select_open: queries on device %d, selection on device %d",
              queries->device, device);
    return -2;
  }
  // the query Multiseq: sequence i starts at the sum of (length_j + 1), j < i
  // (kurtz-basic/multiseq.c:129-166)
  std::vector<uint64_t> qstart, qlen;
  const uint64_t *pstart = layout->querystart, *plen = layout->querylength;
  uint64_t nq = layout->numofqueries, seqoffset = 0;
  uint32_t uniformlen = 0;
  if (queries != nullptr && layout->kind != VSA_SINK_SELF)
  {
    nq = queries->nq;
    seqoffset = queries->seqoffset;
    if (queries->uniform && queries->maxlength > 0 &&
        queries->maxlength < 0xFFFFFFFFull)
    {
      uniformlen = (uint32_t) queries->maxlength;
    }
    else
    {
      qstart.resize(nq);
      qlen.resize(nq);
      uint64_t pos = 0;
      for (uint64_t i = 0; i < nq; i++)
      {
        qlen[i] = queries->uniform ? queries->maxlength : queries->hlength[i];
        qstart[i] = pos;
        pos += qlen[i] + 1;
      }
      pstart = qstart.data();
      plen = qlen.data();
    }
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_select *s = new vsa_select();
  s->device = s->layout.device = s->list.device = device;
  s->selfpalindromic = layout->selfpalindromic != 0;
  memset(&s->stats, 0, sizeof s->stats);
  memset(s->worst, 0, sizeof s->worst);
  int rc = vsa_selctx_init(&s->ctx, layout, params, nq, pstart, plen,
                           uniformlen, seqoffset);
  if (rc != 0)
  {
    memset(&s->ctx, 0, sizeof s->ctx);
    delete s;
    return rc;
  }
  // (upload_tables makes drules of ctx.rules and points it to the copies)
  const uint64_t *hstart = s->ctx.rules.qstart, *hlen = s->ctx.rules.qlen;
  rc = s->layout.upload("vsa_select_open", nq, &hstart, &hlen, 0, nullptr);
  if (rc == 0)
  {
    rc = upload_tables(s);
  }
  if (rc != 0)
  {
    vsa_select_close(s);
    return rc;
  }
  *select = s;
  return 0;
}

extern "C" int vsa_select_add(vsa_select *s, const vsa_result *r,
                              int palindromic)
{
  int rc = check_list(s, r, palindromic, "vsa_select_add");
  if (rc < 0)
  {
    return rc;
  }
  s->lastpasses = 0;
  if (rc > 0)
  {
    return 0;
  }
  if ((rc = ensure_tables(s, r)) != 0)
  {
    return rc;
  }
  const uint64_t N = s->ctx.params.bestnumber;
  KeyF kf;
  kf.r = s->drules;
  kf.r.hasworst = N > 0 && s->nsel == N;
  memcpy(kf.r.worst, s->worst, sizeof s->worst);
  kf.matches = r->matches;
  kf.palindromic = palindromic != 0;
  kf.keys = nullptr;
  kf.stride = kf.base = 0;
  kf.src = nullptr;
  kf.lrecs = nullptr;
  kf.lflags = nullptr;
  DevBuf offsets;
  uint64_t totals[4];
  if (tc_count<1, 4>(kf, r->count, offsets, totals) != 0)
  {
    return -100;
  }
  if (totals[1] != 0)
  {
    VSA_ERROR("vsa_select_add: %lu records do not fit the layout (a query "
              "number outside the %lu of the batch, or a match that leaves "
              "its sequence)", (unsigned long) totals[1],
              (unsigned long) s->ctx.rules.nq);
    return -2;
  }
  const uint64_t m = totals[0];
  if (N > 0)
  {
    if (m > 0 && (rc = sel_best(s, r, kf, offsets, m)) != 0)
    {
      return rc;
    }
  }
  else if (m > 0)
  {
    // filters only: the survivors behind the list so far
    if (s->list.reserve(s->list.n + m) != 0)
    {
      return -100;
    }
    kf.lrecs = s->list.recs;
    kf.lflags = s->list.flags;
    kf.base = s->list.n;
    if (tc_emit<1>(kf, r->count, offsets) != 0)
    {
      return -100;
    }
    VSA_HIP(hipStreamSynchronize(nullptr));
    s->list.n += m;
  }
  s->stats.seen += r->count;
  s->stats.rejected += totals[2];
  s->stats.duplicates += totals[3];
  return 0;
}

extern "C" int vsa_select_finish(vsa_select *s, vsa_result **selected)
{
  if (s == nullptr || selected == nullptr)
  {
    VSA_ERROR("vsa_select_finish: NULL argument");
    return -1;
  }
  *selected = nullptr;
  if (enter(s->device) != 0)
  {
    return -100;
  }
  const bool best = s->ctx.params.bestnumber > 0;
  const uint64_t n = best ? s->nsel : s->list.n;
  const vsa_match *recs = best ? s->srecs : s->list.recs;
  s->lastflags.assign(n, 0);
  s->stats.containedremoved = 0;
  DevBuf flags;
  if (n > 0)
  {
    if (best)
    {
      if (flags.alloc(n) != 0)
      {
        return -100;
      }
      k_sel_flags<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
          s->skeys + (uint64_t) (SEL_W - 1) * n, n, flags.as<uint8_t>());
      VSA_HIP(hipGetLastError());
    }
    VSA_HIP(hipMemcpy(s->lastflags.data(), best ? flags.p : s->list.flags, n,
                      hipMemcpyDeviceToHost));
  }
  if (best && s->ctx.params.sortmode != VSA_SORT_NONE && n > 0)
  {
    // the -sort tail on the host: at most N records
    std::vector<vsa_match> h(n);
    std::vector<double> ev(n);
    VSA_HIP(hipMemcpy(h.data(), recs, n * sizeof(vsa_match),
                      hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(ev.data(), s->skeys, n * 8, hipMemcpyDeviceToHost));
    const int64_t kept = vsa_select_sorttail(&s->ctx, h.data(),
                                             s->lastflags.data(), ev.data(),
                                             n, &s->stats.containedremoved);
    if (kept < 0)
    {
      return (int) kept;
    }
    s->lastflags.resize((size_t) kept);
    s->stats.selected = (uint64_t) kept;
    return vsa_result_from_host(h.data(), (uint64_t) kept, s->device,
                                selected);
  }
  vsa_result *res = newresult(s->device);
  if (n > 0)
  {
    if (vsa_dev_alloc((void **) &res->matches, n * sizeof(vsa_match)) != 0)
    {
      delete res;
      return -100;
    }
    if (hipMemcpy(res->matches, recs, n * sizeof(vsa_match),
                  hipMemcpyDeviceToDevice) != hipSuccess ||
        sumlengths(res->matches, n, nullptr, &res->stats.sumlength) != 0)
    {
      VSA_ERROR("vsa_select_finish: copy of the selection failed");
      vsa_result_free(res);
      return -100;
    }
  }
  res->count = n;
  res->stats.count = n;
  s->stats.selected = n;
  *selected = res;
  return 0;
}

extern "C" int vsa_select_flags(const vsa_select *s, uint8_t *palindromic,
                                uint64_t capacity)
{
  if (s == nullptr || (palindromic == nullptr && capacity > 0))
  {
    VSA_ERROR("vsa_select_flags: NULL argument");
    return -1;
  }
  const uint64_t n = std::min<uint64_t>(capacity, s->lastflags.size());
  if (n > 0)
  {
    memcpy(palindromic, s->lastflags.data(), (size_t) n);
  }
  return 0;
}

extern "C" int vsa_select_getstats(const vsa_select *s, vsa_selectstats *stats)
{
  if (s == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_select_getstats: NULL argument");
    return -1;
  }
  *stats = s->stats;
  return 0;
}

extern "C" uint64_t vsa_select_passes(const vsa_select *s)
{
  return s == nullptr ? 0 : s->lastpasses;
}

extern "C" int vsa_select_evalues(vsa_select *s, const vsa_result *r,
                                  int palindromic, double *evalues,
                                  uint64_t capacity)
{
  if (evalues == nullptr && capacity > 0)
  {
    VSA_ERROR("vsa_select_evalues: NULL argument");
    return -1;
  }
  int rc = check_list(s, r, palindromic, "vsa_select_evalues");
  if (rc != 0)
  {
    return rc < 0 ? rc : 0;
  }
  const uint64_t n = std::min(capacity, r->count);
  if (n == 0)
  {
    return 0;
  }
  if ((rc = ensure_tables(s, r)) != 0)
  {
    return rc;
  }
  DevBuf out, bad;
  uint64_t nbad = 0;
  if (out.alloc(n * 8) != 0 || bad.alloc(8) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(bad.p, 0, 8, nullptr));
  k_sel_evalues<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
      s->drules, r->matches, n, palindromic != 0, out.as<double>(),
      bad.as<unsigned long long>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipMemcpy(evalues, out.p, n * 8, hipMemcpyDeviceToHost));
  VSA_HIP(hipMemcpy(&nbad, bad.p, 8, hipMemcpyDeviceToHost));
  if (nbad != 0)
  {
    VSA_ERROR("vsa_select_evalues: %lu records do not fit the layout",
              (unsigned long) nbad);
    return -2;
  }
  return 0;
}
