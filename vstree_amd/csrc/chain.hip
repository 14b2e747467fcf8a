// Chaining on the device: vmatch -pp chain (Vmatch/chainvm.c:29-500,
// kurtz/matsort.c:316-367, kurtz-basic/chain2dim.c:251-1915) on match lists
// that stay in HBM.  The rules -- what a fragment is, which one precedes
// which, with what score, which chains are retrieved -- are chain_rules.h,
// the same text the host compiles; the kernels go through its rule without
// an order of events (vsa_ch_fold / vsa_ch_settle), the host through the
// literal sweep.
//
//   view      k_ch_view, one lane per record of a list: the view of
//             select_rules.h and the sequence numbers of cluster_rules.h give
//             the fragment and (seqnum1, seqnum2); the record and its D/P flag
//             are kept, the caller may free the list.
//   sort      stable radix sorts of the record numbers, least significant
//             key word first: position2, and when the list is grouped
//             (withinborders, more than one pair) seqnum2 and seqnum1.
//             Problem boundaries and tie runs come from adjacent keys, the
//             boundaries through the stable compaction of tile_compact.inc.
//   replay    the reference's quicksort by seqnum2 is not stable for runs of
//             one seqnum1 of more than 10 records; what it does shows only
//             inside a tie run.  The records of such runs that hold a tie
//             are compacted, go to the host, through the restated quicksort
//             (vsa_ch_grouprank), and their ranks come back as one more,
//             least significant key word.  Lists without ties never leave
//             the device.
//   score     by the size of the problem: k_ch_small, one lane per problem
//             of up to 8 fragments; k_ch_wave, one wavefront per problem of up
//             to 64, lane t = fragment t: at step s the score of lane s is
//             final and broadcast with shuffles, the lanes behind fold it --
//             no LDS, no barrier; k_ch_group, one workgroup per problem of up
//             to VSA_CHAIN_MAXGROUP in tiles of 256 fragments: every thread
//             folds the settled fragments before the tile out of LDS chunks,
//             then the tile settles itself by the same step and broadcast
//             through LDS, one barrier per fragment.
//   retrieve  element-wise with atomics: chain ends, the greatest end score
//             of every problem, the greatest score of every class and its
//             first taker; the selected ends compacted in order; one lane
//             per chain walks back for the length, an exclusive sum, and a
//             second walk writes the members front to back.
// Record and fragment numbers are 32 bit (the entry points refuse more),
// positions and scores 64 bit.  Nothing is launched on zero elements.
#include "resident_list.hpp"
#include "chain_rules.h"
#include <vector>
#include "tile_compact.inc"

enum
{
  CH_VIEW,
  CH_SORT,
  CH_REPLAY,
  CH_SCORE,
  CH_RETRIEVE
};
static_assert(CH_RETRIEVE + 1 == VSA_CHAIN_STAGES,
              "the header counts the stages");
#define CH_MAXRECORDS 0xFFFFFFFFull
#define CH_TILE 256u
static_assert(CH_TILE == TC_BLOCK, "one thread per fragment of a tile");
// scores in atomicMax: the order of int64_t as that of uint64_t
#define CH_FLIP ((uint64_t) 1 << 63)

struct vsa_chain
{
  static constexpr const char *finishname = "vsa_chain_finish";
  int device = 0;
  vsa_selrules view; // the query Multiseq and markpos in device memory
  vsa_clrules seqs;
  DeviceLayout layout;
  vsa_chainparams params;
  // the records so far with their fragments and sequence numbers, and how
  // many of them the last finish saw
  ResidentList list;
  uint64_t nfinished = 0;
  vsa_chfrag *frag = nullptr;
  uint64_t *seq1 = nullptr, *seq2 = nullptr;
  uint64_t *maxima = nullptr; // the largest position2, seqnum1, seqnum2
  // the chains of the last finish
  bool finished = false, everfinished = false, gathered = false;
  std::vector<uint64_t> problem, number, start, hmembers;
  std::vector<int64_t> score;
  uint32_t *members = nullptr; // record numbers, device
  std::vector<vsa_match> memberrecs;
  vsa_chainstats stats;
  double ms[VSA_CHAIN_STAGES] = {0, 0, 0, 0, 0};
};

namespace
{

__device__ __forceinline__ uint64_t ch_wavemax(uint64_t v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const uint64_t o = vsa_shfl64(v, (int) ((threadIdx.x & 63u) ^ (uint32_t) d));
    v = o > v ? o : v;
  }
  return v;
}

// ---- view -----------------------------------------------------------------------

__global__ void __launch_bounds__(TC_BLOCK)
k_ch_view(vsa_selrules view, vsa_clrules seqs, double wf,
          const vsa_match *__restrict__ in, uint64_t n, int palindromic,
          uint64_t base, vsa_match *__restrict__ recs,
          uint8_t *__restrict__ flags, vsa_chfrag *__restrict__ frag,
          uint64_t *__restrict__ seq1, uint64_t *__restrict__ seq2,
          unsigned long long *__restrict__ maxima,
          unsigned long long *__restrict__ bad)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  bool isbad = false;
  uint64_t m0 = 0, m1 = 0, m2 = 0;
  if (i < n)
  {
    const vsa_match m = in[i];
    vsa_chfrag f;
    uint64_t s1, s2;
    if (vsa_ch_view(&view, &seqs, wf, &m, palindromic, &f, &s1, &s2) != 0)
    {
      isbad = true;
    }
    else
    {
      const uint64_t at = base + i;
      recs[at] = m;
      flags[at] = (uint8_t) (palindromic != 0);
      frag[at] = f;
      seq1[at] = s1;
      seq2[at] = s2;
      m0 = f.s1;
      m1 = s1;
      m2 = s2;
    }
  }
  m0 = ch_wavemax(m0);
  m1 = ch_wavemax(m1);
  m2 = ch_wavemax(m2);
  if ((threadIdx.x & 63u) == 0)
  {
    atomicMax(&maxima[0], (unsigned long long) m0);
    atomicMax(&maxima[1], (unsigned long long) m1);
    atomicMax(&maxima[2], (unsigned long long) m2);
  }
  wave_count(isbad, bad);
}

// *differs != 0: some record lies in another pair than record 0
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_onepair(const uint64_t *__restrict__ seq1,
             const uint64_t *__restrict__ seq2, uint64_t n,
             unsigned int *__restrict__ differs)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  const bool d = i < n && (seq1[i] != seq1[0] || seq2[i] != seq2[0]);
  if (__ballot(d) != 0 && (threadIdx.x & 63u) == 0)
  {
    atomicOr(differs, 1u);
  }
}

// ---- sort -----------------------------------------------------------------------

enum
{
  KEY_POSITION2,
  KEY_SEQ2,
  KEY_SEQ1,
  KEY_LAST
};

// key[t] = one word of the key of the record at place t
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_key(int which, const vsa_chfrag *__restrict__ frag,
         const uint64_t *__restrict__ seq1, const uint64_t *__restrict__ seq2,
         const uint32_t *__restrict__ last, const uint32_t *__restrict__ idx,
         uint64_t n, uint64_t *__restrict__ key)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint32_t m = idx[t];
    key[t] = which == KEY_POSITION2
                 ? frag[m].s1
                 : which == KEY_SEQ2 ? seq2[m]
                                     : which == KEY_SEQ1 ? seq1[m] : last[m];
  }
}

// the records in sorted order
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_sorted(const vsa_chfrag *__restrict__ frag,
            const uint64_t *__restrict__ seq1,
            const uint64_t *__restrict__ seq2,
            const uint32_t *__restrict__ idx, uint64_t n,
            vsa_chfrag *__restrict__ sfrag, uint64_t *__restrict__ sseq1,
            uint64_t *__restrict__ sseq2)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint32_t m = idx[t];
    sfrag[t] = frag[m];
    sseq1[t] = seq1[m];
    sseq2[t] = seq2[m];
  }
}

__device__ __forceinline__ bool ch_head(int grouped,
                                        const uint64_t *__restrict__ sseq1,
                                        const uint64_t *__restrict__ sseq2,
                                        uint64_t t)
{
  return t == 0 || (grouped && (sseq1[t] != sseq1[t - 1] ||
                                sseq2[t] != sseq2[t - 1]));
}

// place t ties with the one before it
__device__ __forceinline__ bool ch_tie(int grouped,
                                       const vsa_chfrag *__restrict__ sfrag,
                                       const uint64_t *__restrict__ sseq1,
                                       const uint64_t *__restrict__ sseq2,
                                       uint64_t t)
{
  return t > 0 && !ch_head(grouped, sseq1, sseq2, t) &&
         sfrag[t].s1 == sfrag[t - 1].s1;
}

// class 0: the first fragment of a problem (its place is stored); class 1:
// the second record of a tie run (counted)
struct HeadF
{
  typedef NoPayload Payload;
  int grouped;
  const vsa_chfrag *sfrag;
  const uint64_t *sseq1, *sseq2;
  uint64_t *pstart;

  __device__ int cls(uint64_t t, Payload &) const
  {
    if (ch_head(grouped, sseq1, sseq2, t))
    {
      return 0;
    }
    return ch_tie(grouped, sfrag, sseq1, sseq2, t) &&
                   !ch_tie(grouped, sfrag, sseq1, sseq2, t - 1)
               ? 1
               : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t t, const Payload &) const
  {
    pstart[rank] = t;
  }
};

// ---- replay ---------------------------------------------------------------------

// runflag[lo] = 1 for the first place lo of every run of one seqnum1 of more
// than VSA_CH_STABLEWIDTH records that holds a tie
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_markruns(const vsa_chfrag *__restrict__ sfrag,
              const uint64_t *__restrict__ sseq1,
              const uint64_t *__restrict__ sseq2, uint64_t n,
              uint8_t *__restrict__ runflag)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t < n && ch_tie(1, sfrag, sseq1, sseq2, t))
  {
    const uint64_t s = sseq1[t], lo = vsa_lowerbound(sseq1, n, s);
    uint64_t hi = lo + VSA_CH_STABLEWIDTH;
    if (hi < n && sseq1[hi] == s)
    {
      runflag[lo] = 1;
    }
  }
}

// the records of the marked runs, in sorted order
struct ReplayF
{
  typedef NoPayload Payload;
  const uint64_t *sseq1, *sseq2;
  const uint32_t *sidx;
  const uint8_t *runflag;
  uint64_t n;
  uint64_t *oseq1, *oseq2;
  uint32_t *orec;

  __device__ int cls(uint64_t t, Payload &) const
  {
    return runflag[vsa_lowerbound(sseq1, n, sseq1[t])] ? 0 : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t t, const Payload &) const
  {
    oseq1[rank] = sseq1[t];
    oseq2[rank] = sseq2[t];
    orec[rank] = sidx[t];
  }
};

// last[rec[k]] = rank[k]
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_scatter(const uint32_t *__restrict__ rec,
             const uint32_t *__restrict__ rank, uint64_t k,
             uint32_t *__restrict__ last)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t < k)
  {
    last[rec[t]] = rank[t];
  }
}

// ---- problems -------------------------------------------------------------------

// *largest = the fragments of the largest problem
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_largest(const uint64_t *__restrict__ pstart, uint64_t nproblems,
             unsigned long long *__restrict__ largest)
{
  const uint64_t p = vsa_bid() * TC_BLOCK + threadIdx.x;
  const uint64_t size =
      ch_wavemax(p < nproblems ? pstart[p + 1] - pstart[p] : 0);
  if ((threadIdx.x & 63u) == 0)
  {
    atomicMax(largest, (unsigned long long) size);
  }
}

// the problems by class of size, in order
struct ClassF
{
  typedef NoPayload Payload;
  const uint64_t *pstart;
  uint64_t nproblems;
  uint32_t *list; // VSA_CH_CLASSES lists of nproblems entries
  uint32_t smallmax, wavemax;

  __device__ int cls(uint64_t p, Payload &) const
  {
    return vsa_ch_classof(pstart[p + 1] - pstart[p], smallmax, wavemax);
  }
  __device__ void put(int c, uint64_t rank, uint64_t p, const Payload &) const
  {
    list[(uint64_t) c * nproblems + rank] = (uint32_t) p;
  }
};

// pid[t] = the problem of place t
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_pid(const uint64_t *__restrict__ pstart, uint64_t nproblems, uint64_t n,
         uint32_t *__restrict__ pid)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t < n)
  {
    // the last problem that starts at t or before it
    pid[t] = (uint32_t) (vsa_lowerbound(pstart, nproblems, t + 1) - 1);
  }
}

// ---- score ----------------------------------------------------------------------

// the arrays of the fragments in sorted order
struct Frags
{
  const vsa_chfrag *f;
  int64_t *tg, *score;
  uint32_t *prev, *first; // numbers within the problem
};

__device__ __forceinline__ void ch_cand(const Frags &a, uint64_t t,
                                        vsa_chcand &c)
{
  const vsa_chfrag f = a.f[t];
  c.s0 = f.s0;
  c.e0 = f.e0;
  c.s1 = f.s1;
  c.e1 = f.e1;
  c.score = a.score[t];
  c.tg = a.tg[t];
  c.first = a.first[t];
}

__device__ __forceinline__ void ch_nobest(vsa_chbest &b)
{
  b.has = b.link = 0;
  b.key = b.score = 0;
  b.e0 = b.e1 = 0;
  b.j = b.first = 0;
}

// one lane per problem of 2 .. VSA_CH_SMALLMAX fragments
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_small(vsa_chainparams r, Frags a, const uint64_t *__restrict__ pstart,
           const uint32_t *__restrict__ list, uint64_t count)
{
  const uint64_t k = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (k >= count)
  {
    return;
  }
  const uint64_t b = pstart[list[k]];
  const uint32_t n = (uint32_t) (pstart[list[k] + 1] - b);
  uint64_t big0 = 0, big1 = 0;
  for (uint32_t i = 0; i < n; i++)
  {
    const vsa_chfrag f = a.f[b + i];
    big0 = f.e0 > big0 ? f.e0 : big0;
    big1 = f.e1 > big1 ? f.e1 : big1;
  }
  for (uint32_t i = 0; i < n; i++)
  {
    const vsa_chfrag f = a.f[b + i];
    vsa_chbest best;
    ch_nobest(best);
    a.tg[b + i] = vsa_ch_terminalgap(r.kind, big0, big1, f.e0, f.e1);
    for (uint32_t j = 0; j < i; j++)
    {
      vsa_chcand c;
      ch_cand(a, b + j, c);
      vsa_ch_fold(&r, &best, &c, j, &f);
    }
    vsa_ch_settle(&r, &best, &f, i, &a.score[b + i], &a.prev[b + i],
                  &a.first[b + i]);
  }
}

// one wavefront per problem of up to VSA_CH_WAVEMAX fragments, lane t =
// fragment t
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_wave(vsa_chainparams r, Frags a, const uint64_t *__restrict__ pstart,
          const uint32_t *__restrict__ list, uint64_t count)
{
  const uint64_t k = vsa_bid() * (TC_BLOCK / 64) + (threadIdx.x >> 6);
  if (k >= count)
  {
    return; // the whole wavefront
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t b = pstart[list[k]];
  const uint32_t n = (uint32_t) (pstart[list[k] + 1] - b);
  const bool mine = lane < n;
  vsa_chfrag f = {0, 0, 0, 0, 0};
  if (mine)
  {
    f = a.f[b + lane];
  }
  const uint64_t big0 = ch_wavemax(f.e0), big1 = ch_wavemax(f.e1);
  const int64_t tg = vsa_ch_terminalgap(r.kind, big0, big1, f.e0, f.e1);
  int64_t score = 0;
  uint32_t prev = VSA_CHAIN_NONE, first = lane;
  vsa_chbest best;
  ch_nobest(best);
  for (uint32_t s = 0; s < n; s++)
  {
    if (lane == s)
    {
      vsa_ch_settle(&r, &best, &f, lane, &score, &prev, &first);
    }
    vsa_chcand c;
    c.s0 = vsa_shfl64(f.s0, (int) s);
    c.e0 = vsa_shfl64(f.e0, (int) s);
    c.s1 = vsa_shfl64(f.s1, (int) s);
    c.e1 = vsa_shfl64(f.e1, (int) s);
    c.score = (int64_t) vsa_shfl64((uint64_t) score, (int) s);
    c.tg = (int64_t) vsa_shfl64((uint64_t) tg, (int) s);
    c.first = __shfl(first, (int) s, 64);
    if (mine && lane > s)
    {
      vsa_ch_fold(&r, &best, &c, s, &f);
    }
  }
  if (mine)
  {
    a.tg[b + lane] = tg;
    a.score[b + lane] = score;
    a.prev[b + lane] = prev;
    a.first[b + lane] = first;
  }
}

// one workgroup per problem of up to VSA_CHAIN_MAXGROUP fragments
__global__ void __launch_bounds__(CH_TILE)
k_ch_group(vsa_chainparams r, Frags a, const uint64_t *__restrict__ pstart,
           const uint32_t *__restrict__ list, uint64_t count)
{
  if (vsa_bid() >= count)
  {
    return; // the whole workgroup
  }
  __shared__ uint64_t sh_s0[CH_TILE], sh_e0[CH_TILE], sh_s1[CH_TILE],
      sh_e1[CH_TILE];
  __shared__ int64_t sh_score[CH_TILE], sh_tg[CH_TILE];
  __shared__ uint32_t sh_first[CH_TILE];
  __shared__ uint64_t sh_big[2 * (CH_TILE / 64)];
  const uint32_t tid = threadIdx.x;
  const uint64_t b = pstart[list[vsa_bid()]];
  const uint32_t n = (uint32_t) (pstart[list[vsa_bid()] + 1] - b);

  uint64_t big0 = 0, big1 = 0;
  for (uint32_t i = tid; i < n; i += CH_TILE)
  {
    const vsa_chfrag f = a.f[b + i];
    big0 = f.e0 > big0 ? f.e0 : big0;
    big1 = f.e1 > big1 ? f.e1 : big1;
  }
  big0 = ch_wavemax(big0);
  big1 = ch_wavemax(big1);
  if ((tid & 63u) == 0)
  {
    sh_big[2 * (tid >> 6)] = big0;
    sh_big[2 * (tid >> 6) + 1] = big1;
  }
  __syncthreads();
  for (uint32_t w = 0; w < CH_TILE / 64; w++)
  {
    big0 = sh_big[2 * w] > big0 ? sh_big[2 * w] : big0;
    big1 = sh_big[2 * w + 1] > big1 ? sh_big[2 * w + 1] : big1;
  }
  for (uint32_t i = tid; i < n; i += CH_TILE)
  {
    const vsa_chfrag f = a.f[b + i];
    a.tg[b + i] = vsa_ch_terminalgap(r.kind, big0, big1, f.e0, f.e1);
  }
  for (uint32_t base = 0; base < n; base += CH_TILE)
  {
    const uint32_t i = base + tid;
    const bool mine = i < n;
    const uint32_t steps = n - base < CH_TILE ? n - base : CH_TILE;
    vsa_chfrag f = {0, 0, 0, 0, 0};
    int64_t tg = 0;
    vsa_chbest best;
    ch_nobest(best);
    if (mine)
    {
      f = a.f[b + i];
      tg = vsa_ch_terminalgap(r.kind, big0, big1, f.e0, f.e1);
    }
    // the settled fragments before the tile, CH_TILE of them at a time
    for (uint32_t cb = 0; cb < base; cb += CH_TILE)
    {
      vsa_chcand c;
      __syncthreads(); // the chunk before has been read; scores are written
      ch_cand(a, b + cb + tid, c); // cb + tid < base <= n
      sh_s0[tid] = c.s0;
      sh_e0[tid] = c.e0;
      sh_s1[tid] = c.s1;
      sh_e1[tid] = c.e1;
      sh_score[tid] = c.score;
      sh_tg[tid] = c.tg;
      sh_first[tid] = c.first;
      __syncthreads();
      if (mine)
      {
        for (uint32_t j = 0; j < CH_TILE; j++)
        {
          c.s0 = sh_s0[j];
          c.e0 = sh_e0[j];
          c.s1 = sh_s1[j];
          c.e1 = sh_e1[j];
          c.score = sh_score[j];
          c.tg = sh_tg[j];
          c.first = sh_first[j];
          vsa_ch_fold(&r, &best, &c, cb + j, &f);
        }
      }
    }
    __syncthreads();
    // the tile itself: fragment base + s is settled at step s
    for (uint32_t s = 0; s < steps; s++)
    {
      if (tid == s)
      {
        int64_t score;
        uint32_t prev, first;
        vsa_ch_settle(&r, &best, &f, i, &score, &prev, &first);
        a.score[b + i] = score;
        a.prev[b + i] = prev;
        a.first[b + i] = first;
        sh_s0[s] = f.s0;
        sh_e0[s] = f.e0;
        sh_s1[s] = f.s1;
        sh_e1[s] = f.e1;
        sh_score[s] = score;
        sh_tg[s] = tg;
        sh_first[s] = first;
      }
      __syncthreads();
      if (mine && tid > s)
      {
        vsa_chcand c;
        c.s0 = sh_s0[s];
        c.e0 = sh_e0[s];
        c.s1 = sh_s1[s];
        c.e1 = sh_e1[s];
        c.score = sh_score[s];
        c.tg = sh_tg[s];
        c.first = sh_first[s];
        vsa_ch_fold(&r, &best, &c, base + s, &f);
      }
    }
  }
}

// ---- retrieve -------------------------------------------------------------------

struct Retr
{
  vsa_chainparams r;
  Frags a;
  const uint64_t *pstart;
  const uint32_t *pid;
  uint64_t n;
  uint8_t *rm;                // the fragment ends a chain
  unsigned long long *pbest;  // per problem, flipped
  unsigned long long *cbest;  // per class = first fragment, flipped
  uint32_t *ctaker;
  int64_t *kth, *thr; // per problem
};

__device__ __forceinline__ bool ch_single(const Retr &q, uint32_t p)
{
  return q.pstart[p + 1] - q.pstart[p] == 1;
}

// chain ends and the maxima of problems and classes
__global__ void __launch_bounds__(TC_BLOCK) k_ch_ends(Retr q)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t >= q.n)
  {
    return;
  }
  const uint32_t p = q.pid[t];
  const uint64_t b = q.pstart[p], e = q.pstart[p + 1];
  if (e - b == 1)
  {
    q.rm[t] = 1;
    return;
  }
  const int64_t score = q.a.score[t];
  const bool last = t + 1 == e;
  const bool rm = vsa_ch_rightmax(last, last ? 0 : q.a.prev[t + 1],
                                  last ? 0 : q.a.score[t + 1],
                                  (uint32_t) (t - b), score);
  q.rm[t] = rm ? 1 : 0;
  if (q.r.kind == VSA_CHAIN_GLOBAL)
  {
    atomicMax(&q.pbest[p], (unsigned long long) ((uint64_t) score ^ CH_FLIP));
  }
  else if (rm)
  {
    const int64_t es = vsa_ch_endscore(q.r.kind, score, q.a.tg[t]);
    atomicMax(&q.pbest[p], (unsigned long long) ((uint64_t) es ^ CH_FLIP));
    if (vsa_ch_islocal(q.r.kind))
    {
      atomicMax(&q.cbest[b + q.a.first[t]],
                (unsigned long long) ((uint64_t) score ^ CH_FLIP));
    }
  }
}

// local Kb: one wavefront per problem finds the K-th largest distinct score
// of its chain ends, compared as unsigned numbers (dictmaxsize.c)
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_kth(Retr q, uint64_t nproblems)
{
  const uint64_t p = vsa_bid() * (TC_BLOCK / 64) + (threadIdx.x >> 6);
  if (p >= nproblems)
  {
    return;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t b = q.pstart[p], e = q.pstart[p + 1];
  uint64_t cur = 0;
  for (int64_t found = 0; found < q.r.value; found++)
  {
    uint64_t m = 0;
    bool any = false;
    for (uint64_t t = b + lane; t < e; t += 64)
    {
      const uint64_t s = (uint64_t) q.a.score[t];
      if (q.rm[t] && (found == 0 || s < cur) && (!any || s > m))
      {
        m = s;
        any = true;
      }
    }
    if (__ballot(any) == 0)
    {
      break;
    }
    // lanes without a value bring 0, which is below or equal to any
    m = ch_wavemax(any ? m : 0);
    cur = m;
  }
  if (lane == 0)
  {
    q.kth[p] = (int64_t) cur;
  }
}

__global__ void __launch_bounds__(TC_BLOCK)
k_ch_threshold(Retr q, uint64_t nproblems)
{
  const uint64_t p = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (p < nproblems)
  {
    q.thr[p] = vsa_ch_threshold(&q.r, (int64_t) (q.pbest[p] ^ CH_FLIP),
                                q.kth[p]);
  }
}

// the first chain end of every class that has the class's greatest score
__global__ void __launch_bounds__(TC_BLOCK) k_ch_takers(Retr q)
{
  const uint64_t t = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (t >= q.n || !q.rm[t])
  {
    return;
  }
  const uint32_t p = q.pid[t];
  if (ch_single(q, p))
  {
    return;
  }
  const uint64_t slot = q.pstart[p] + q.a.first[t];
  if (((uint64_t) q.a.score[t] ^ CH_FLIP) == q.cbest[slot])
  {
    atomicMin(&q.ctaker[slot], (uint32_t) (t - q.pstart[p]));
  }
}

// the ends that give a chain, in order
struct EndF
{
  typedef NoPayload Payload;
  Retr q;
  uint32_t *ends;

  __device__ int cls(uint64_t t, Payload &) const
  {
    if (!q.rm[t])
    {
      return -1;
    }
    const uint32_t p = q.pid[t];
    if (ch_single(q, p))
    {
      return 0; // chainingboundarycases: whatever the threshold
    }
    const int64_t es = vsa_ch_endscore(q.r.kind, q.a.score[t], q.a.tg[t]);
    if (es < q.thr[p])
    {
      return -1;
    }
    if (vsa_ch_islocal(q.r.kind))
    {
      const uint64_t b = q.pstart[p], slot = b + q.a.first[t];
      if (q.ctaker[slot] != (uint32_t) (t - b) ||
          ((uint64_t) es ^ CH_FLIP) != q.cbest[slot])
      {
        return -1;
      }
    }
    return 0;
  }
  __device__ void put(int, uint64_t rank, uint64_t t, const Payload &) const
  {
    ends[rank] = (uint32_t) t;
  }
};

// one lane per chain: problem, number, score and length; one more lane
// writes length[nchains] = 0 for the exclusive sum
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_chains(Retr q, const uint32_t *__restrict__ ends, uint64_t nchains,
            uint64_t *__restrict__ problem, uint64_t *__restrict__ number,
            int64_t *__restrict__ score, uint64_t *__restrict__ length)
{
  const uint64_t c = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (c > nchains)
  {
    return;
  }
  if (c == nchains)
  {
    length[c] = 0;
    return;
  }
  const uint64_t t = ends[c];
  const uint32_t p = q.pid[t];
  const uint64_t b = q.pstart[p];
  problem[c] = p;
  number[c] = c - vsa_lowerbound(ends, nchains, b);
  if (ch_single(q, p))
  {
    const vsa_chfrag f = q.a.f[t];
    score[c] = vsa_ch_single(q.r.kind, &f);
    length[c] = 1;
    return;
  }
  score[c] = vsa_ch_endscore(q.r.kind, q.a.score[t], q.a.tg[t]);
  uint64_t len = 0;
  // (a chain has at most as many members as its problem has fragments)
  for (uint32_t i = (uint32_t) (t - b);
       i != VSA_CHAIN_NONE && len < q.pstart[p + 1] - b; i = q.a.prev[b + i])
  {
    len++;
  }
  length[c] = len;
}

// the second walk: the members front to back, as record numbers
__global__ void __launch_bounds__(TC_BLOCK)
k_ch_members(Retr q, const uint32_t *__restrict__ ends, uint64_t nchains,
             const uint64_t *__restrict__ start,
             const uint32_t *__restrict__ sidx, uint32_t *__restrict__ members)
{
  const uint64_t c = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (c >= nchains)
  {
    return;
  }
  const uint64_t t = ends[c], b = q.pstart[q.pid[t]];
  uint64_t k = start[c + 1];
  if (ch_single(q, q.pid[t]))
  {
    members[start[c]] = sidx[t];
    return;
  }
  for (uint32_t i = (uint32_t) (t - b); i != VSA_CHAIN_NONE && k > start[c];
       i = q.a.prev[b + i])
  {
    members[--k] = sidx[b + i];
  }
}

// ---- host -----------------------------------------------------------------------

// the largest problem of a class: the constant of chain_rules.h, or for the
// measurement of scripts/chain_probe.py what the environment says (a lane
// takes any size, a wavefront at most 64 fragments)
uint32_t classbound(const char *name, uint32_t preset, uint32_t least)
{
  const char *s = getenv(name);
  if (s != nullptr && *s != '\0')
  {
    char *end = nullptr;
    const unsigned long v = strtoul(s, &end, 10);
    if (*end == '\0' && v >= least && v <= VSA_CH_WAVEMAX)
    {
      return (uint32_t) v;
    }
  }
  return preset;
}

// the order of the records: place t holds record idx[t]
struct Sorter
{
  const vsa_chain *c;
  DevBuf idx, idx2, key, key2;

  int init()
  {
    const uint64_t n = c->list.n;
    if (idx.alloc(n * 4) != 0 || idx2.alloc(n * 4) != 0 ||
        key.alloc(n * 8) != 0 || key2.alloc(n * 8) != 0)
    {
      return -100;
    }
    k_tc_iota<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(idx.as<uint32_t>(), n);
    VSA_HIP(hipGetLastError());
    return 0;
  }
  // a stable sort by one word of the key, of which `bits` bits count
  int pass(int which, unsigned int bits, const uint32_t *last)
  {
    const uint64_t n = c->list.n;
    k_ch_key<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
        which, c->frag, c->seq1, c->seq2, last, idx.as<uint32_t>(), n,
        key.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    if (sortpairs(key.as<uint64_t>(), key2.as<uint64_t>(), idx.as<uint32_t>(),
                  idx2.as<uint32_t>(), n, bits, nullptr) != 0)
    {
      return -100;
    }
    std::swap(idx.p, idx2.p);
    return 0;
  }
  int sort(int grouped, const uint64_t *maxima, const uint32_t *last)
  {
    if ((last != nullptr && pass(KEY_LAST, 32, last) != 0) ||
        pass(KEY_POSITION2, bitsfor(maxima[0]), nullptr) != 0 ||
        (grouped && (pass(KEY_SEQ2, bitsfor(maxima[2]), nullptr) != 0 ||
                     pass(KEY_SEQ1, bitsfor(maxima[1]), nullptr) != 0)))
    {
      return -100;
    }
    return 0;
  }
};

// the members and their records into host memory, once per finish
int hostmembers(vsa_chain *c)
{
  if (c->gathered)
  {
    return 0;
  }
  const uint64_t k = c->stats.chained;
  c->hmembers.resize(k);
  if (members_to_host(c->list, c->members, k, c->memberrecs) != 0)
  {
    return -100;
  }
  if (k > 0)
  {
    std::vector<uint32_t> h(k);
    VSA_HIP(hipMemcpy(h.data(), c->members, k * 4, hipMemcpyDeviceToHost));
    for (uint64_t t = 0; t < k; t++)
    {
      c->hmembers[t] = h[t];
    }
  }
  c->gathered = true;
  return 0;
}

} // namespace

extern "C" void vsa_chain_close(vsa_chain *c)
{
  if (c == nullptr)
  {
    return;
  }
  c->layout.release();
  c->list.release();
  vsa_dev_free(c->maxima);
  vsa_dev_free(c->members);
  delete c;
}

extern "C" int vsa_chain_open(const vsa_sinkparams *layout,
                              const vsa_chainparams *params, int device,
                              vsa_chain **chain)
{
  if (chain == nullptr)
  {
    VSA_ERROR("vsa_chain_open: NULL argument");
    return -1;
  }
  *chain = nullptr;
  vsa_selrules view;
  vsa_clrules seqs;
  const int rc = vsa_ch_checklayout(layout, params, "vsa_chain_open", &view,
                                    &seqs);
  if (rc != 0)
  {
    return rc;
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_chain *c = new vsa_chain();
  c->device = c->layout.device = c->list.device = device;
  c->list.column(&c->frag);
  c->list.column(&c->seq1);
  c->list.column(&c->seq2);
  c->view = view;
  c->seqs = seqs;
  c->params = *params;
  memset(&c->stats, 0, sizeof c->stats);
  if (c->layout.upload("vsa_chain_open", view.nq, &c->view.qstart,
                       &c->view.qlen, seqs.numofsequences - 1,
                       &c->seqs.markpos) != 0 ||
      vsa_dev_alloc((void **) &c->maxima, 3 * 8) != 0 ||
      hipMemset(c->maxima, 0, 3 * 8) != hipSuccess)
  {
    vsa_chain_close(c);
    return -100;
  }
  *chain = c;
  return 0;
}

extern "C" int vsa_chain_add(vsa_chain *c, const vsa_result *r,
                             int palindromic)
{
  const int g = gate("vsa_chain_add", "chain", "chaining", c, r,
                     [&]() { return selfform(c->view.kind, palindromic); },
                     CH_MAXRECORDS, "records: only fewer than 2^32 - 1");
  if (g != 0)
  {
    return g < 0 ? g : 0;
  }
  ScratchWords scratch; // the maxima with this list, and the bad records
  if (c->list.reserve(c->list.n + r->count) != 0 || scratch.alloc(4) != 0)
  {
    return -100;
  }
  Timer t(nullptr);
  t.start();
  VSA_HIP(hipMemcpyAsync(scratch.word(0), c->maxima, 3 * 8,
                         hipMemcpyDeviceToDevice, nullptr));
  if (scratch.zero(3, 1) != 0)
  {
    return -100;
  }
  k_ch_view<<<gridfor(r->count), TC_BLOCK, 0, nullptr>>>(
      c->view, c->seqs, c->params.weightfactor, r->matches, r->count,
      palindromic != 0, c->list.n, c->list.recs, c->list.flags, c->frag,
      c->seq1, c->seq2, scratch.word(0), scratch.word(3));
  VSA_HIP(hipGetLastError());
  t.stop();
  uint64_t nbad = 0;
  if (scratch.fetch(3, 1, &nbad) != 0)
  {
    return -100;
  }
  c->ms[CH_VIEW] += t.ms();
  if (nbad != 0)
  {
    return misfits("vsa_chain_add", nbad,
                   "a query number outside the set, a match that leaves its "
                   "sequence or the text");
  }
  VSA_HIP(hipMemcpy(c->maxima, scratch.word(0), 3 * 8,
                    hipMemcpyDeviceToDevice));
  c->list.n += r->count;
  c->finished = false;
  return 0;
}

extern "C" int vsa_chain_finish(vsa_chain *c)
{
  if (c == nullptr)
  {
    VSA_ERROR("vsa_chain_finish: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0)
  {
    return -100;
  }
  const uint64_t n = c->list.n;
  vsa_chainstats st;
  memset(&st, 0, sizeof st);
  st.matches = n;
  std::vector<uint64_t> hproblem, hnumber, hstart(1, 0);
  std::vector<int64_t> hscore;
  DevBuf members;
  double ms[VSA_CHAIN_STAGES] = {0, 0, 0, 0, 0};
  if (n > 0)
  {
    Timer tsort(nullptr), treplay(nullptr), tscore(nullptr), tretr(nullptr);
    uint64_t maxima[3];
    unsigned int differs = 0;
    DevBuf word, sfrag, sseq1, sseq2, pstart, offsets;
    Sorter srt;
    srt.c = c;
    // ---- sort
    tsort.start();
    if (word.alloc(8) != 0 || sfrag.alloc(n * sizeof(vsa_chfrag)) != 0 ||
        sseq1.alloc(n * 8) != 0 || sseq2.alloc(n * 8) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(word.p, 0, 8, nullptr));
    k_ch_onepair<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
        c->seq1, c->seq2, n, word.as<unsigned int>());
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(&differs, word.p, 4, hipMemcpyDeviceToHost));
    VSA_HIP(hipMemcpy(maxima, c->maxima, 3 * 8, hipMemcpyDeviceToHost));
    // vmatchchaining, chainvm.c:471-497
    const int grouped = c->params.withinborders && differs != 0;
    if (srt.init() != 0 || srt.sort(grouped, maxima, nullptr) != 0)
    {
      return -100;
    }
    k_ch_sorted<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
        c->frag, c->seq1, c->seq2, srt.idx.as<uint32_t>(), n,
        sfrag.as<vsa_chfrag>(), sseq1.as<uint64_t>(), sseq2.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    HeadF hf = {grouped, sfrag.as<vsa_chfrag>(), sseq1.as<uint64_t>(),
                sseq2.as<uint64_t>(), nullptr};
    uint64_t totals[2];
    if (tc_count<1, 2>(hf, n, offsets, totals) != 0)
    {
      return -100;
    }
    const uint64_t np = totals[0];
    st.problems = np;
    st.tieruns = totals[1];
    if (pstart.alloc((np + 1) * 8) != 0)
    {
      return -100;
    }
    hf.pstart = pstart.as<uint64_t>();
    if (tc_emit<1>(hf, n, offsets) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemcpyAsync(pstart.as<uint64_t>() + np, &n, 8,
                           hipMemcpyHostToDevice, nullptr));
    VSA_HIP(hipStreamSynchronize(nullptr));
    tsort.stop();
    // ---- replay
    if (grouped && st.tieruns > 0)
    {
      DevBuf runflag, roff, oseq1, oseq2, orec;
      uint64_t k = 0;
      treplay.start();
      if (runflag.alloc(n) != 0)
      {
        return -100;
      }
      VSA_HIP(hipMemsetAsync(runflag.p, 0, n, nullptr));
      k_ch_markruns<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
          sfrag.as<vsa_chfrag>(), sseq1.as<uint64_t>(), sseq2.as<uint64_t>(),
          n, runflag.as<uint8_t>());
      VSA_HIP(hipGetLastError());
      ReplayF rf = {sseq1.as<uint64_t>(), sseq2.as<uint64_t>(),
                    srt.idx.as<uint32_t>(), runflag.as<uint8_t>(), n, nullptr,
                    nullptr, nullptr};
      if (tc_count<1, 1>(rf, n, roff, &k) != 0)
      {
        return -100;
      }
      st.replayed = k;
      if (k > 0)
      {
        std::vector<uint64_t> h1(k), h2(k);
        std::vector<uint32_t> hrec(k), hrank(k);
        DevBuf last, drank;
        if (oseq1.alloc(k * 8) != 0 || oseq2.alloc(k * 8) != 0 ||
            orec.alloc(k * 4) != 0 || last.alloc(n * 4) != 0 ||
            drank.alloc(k * 4) != 0)
        {
          return -100;
        }
        rf.oseq1 = oseq1.as<uint64_t>();
        rf.oseq2 = oseq2.as<uint64_t>();
        rf.orec = orec.as<uint32_t>();
        if (tc_emit<1>(rf, n, roff) != 0)
        {
          return -100;
        }
        VSA_HIP(hipMemcpy(h1.data(), oseq1.p, k * 8, hipMemcpyDeviceToHost));
        VSA_HIP(hipMemcpy(h2.data(), oseq2.p, k * 8, hipMemcpyDeviceToHost));
        VSA_HIP(hipMemcpy(hrec.data(), orec.p, k * 4, hipMemcpyDeviceToHost));
        const int rc = vsa_ch_grouprank(h1.data(), h2.data(), hrec.data(), k,
                                        hrank.data());
        if (rc != 0)
        {
          return rc;
        }
        VSA_HIP(hipMemcpy(drank.p, hrank.data(), k * 4,
                          hipMemcpyHostToDevice));
        // the record number is the last key word of all other records: a
        // tie run lies in one run of one seqnum1, replayed as a whole or not
        k_tc_iota<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(last.as<uint32_t>(),
                                                        n);
        VSA_HIP(hipGetLastError());
        k_ch_scatter<<<gridfor(k), TC_BLOCK, 0, nullptr>>>(
            orec.as<uint32_t>(), drank.as<uint32_t>(), k,
            last.as<uint32_t>());
        VSA_HIP(hipGetLastError());
        if (srt.init() != 0 ||
            srt.sort(grouped, maxima, last.as<uint32_t>()) != 0)
        {
          return -100;
        }
        // (the keys are the same: the problems start where they did)
        k_ch_sorted<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(
            c->frag, c->seq1, c->seq2, srt.idx.as<uint32_t>(), n,
            sfrag.as<vsa_chfrag>(), sseq1.as<uint64_t>(),
            sseq2.as<uint64_t>());
        VSA_HIP(hipGetLastError());
        VSA_HIP(hipStreamSynchronize(nullptr));
      }
      treplay.stop();
    }
    // ---- score
    tscore.start();
    DevBuf list, coff, tg, score, prev, first;
    uint64_t ctot[VSA_CH_CLASSES];
    if (list.alloc(VSA_CH_CLASSES * np * 4) != 0 || tg.alloc(n * 8) != 0 ||
        score.alloc(n * 8) != 0 || prev.alloc(n * 4) != 0 ||
        first.alloc(n * 4) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(word.p, 0, 8, nullptr));
    VSA_HIP(hipMemsetAsync(tg.p, 0, n * 8, nullptr));
    VSA_HIP(hipMemsetAsync(score.p, 0, n * 8, nullptr));
    VSA_HIP(hipMemsetAsync(prev.p, 0xFF, n * 4, nullptr));
    VSA_HIP(hipMemsetAsync(first.p, 0, n * 4, nullptr));
    const uint32_t smallmax = classbound("VSA_CHAIN_SMALLMAX",
                                         VSA_CH_SMALLMAX, 1);
    const ClassF cf = {pstart.as<uint64_t>(), np, list.as<uint32_t>(),
                       smallmax,
                       classbound("VSA_CHAIN_WAVEMAX", VSA_CH_WAVEMAX,
                                  smallmax)};
    k_ch_largest<<<gridfor(np), TC_BLOCK, 0, nullptr>>>(
        pstart.as<uint64_t>(), np, word.as<unsigned long long>());
    VSA_HIP(hipGetLastError());
    if (tc_count<VSA_CH_CLASSES, VSA_CH_CLASSES>(cf, np, coff, ctot) != 0)
    {
      return -100;
    }
    uint64_t largest = 0;
    VSA_HIP(hipMemcpy(&largest, word.p, 8, hipMemcpyDeviceToHost));
    if (largest > VSA_CHAIN_MAXGROUP)
    {
      VSA_ERROR("vsa_chain_finish: a problem of %lu fragments: the device "
                "covers at most %lu (vsa_chain_host takes any size)",
                (unsigned long) largest, (unsigned long) VSA_CHAIN_MAXGROUP);
      // back to the last finish: its chains stay, the lists since then go
      c->list.n = c->nfinished;
      c->finished = c->everfinished;
      return VSA_NOT_COVERED;
    }
    if (tc_emit<VSA_CH_CLASSES>(cf, np, coff) != 0)
    {
      return -100;
    }
    st.single = ctot[VSA_CH_SINGLE];
    st.small = ctot[VSA_CH_SMALL];
    st.wave = ctot[VSA_CH_WAVE];
    st.group = ctot[VSA_CH_GROUP];
    st.largest = largest;
    const Frags fr = {sfrag.as<vsa_chfrag>(), tg.as<int64_t>(),
                      score.as<int64_t>(), prev.as<uint32_t>(),
                      first.as<uint32_t>()};
    if (st.small > 0)
    {
      k_ch_small<<<gridfor(st.small), TC_BLOCK, 0, nullptr>>>(
          c->params, fr, pstart.as<uint64_t>(),
          list.as<uint32_t>() + VSA_CH_SMALL * np, st.small);
      VSA_HIP(hipGetLastError());
    }
    if (st.wave > 0)
    {
      k_ch_wave<<<vsa_grid((st.wave + TC_BLOCK / 64 - 1) / (TC_BLOCK / 64)),
                  TC_BLOCK, 0, nullptr>>>(
          c->params, fr, pstart.as<uint64_t>(),
          list.as<uint32_t>() + VSA_CH_WAVE * np, st.wave);
      VSA_HIP(hipGetLastError());
    }
    if (st.group > 0)
    {
      k_ch_group<<<vsa_grid(st.group), CH_TILE, 0, nullptr>>>(
          c->params, fr, pstart.as<uint64_t>(),
          list.as<uint32_t>() + VSA_CH_GROUP * np, st.group);
      VSA_HIP(hipGetLastError());
    }
    tscore.stop();
    // ---- retrieve
    tretr.start();
    DevBuf pid, rm, pbest, cbest, ctaker, kth, thr, eoff, ends;
    if (pid.alloc(n * 4) != 0 || rm.alloc(n) != 0 || pbest.alloc(np * 8) != 0 ||
        cbest.alloc(n * 8) != 0 || ctaker.alloc(n * 4) != 0 ||
        kth.alloc(np * 8) != 0 || thr.alloc(np * 8) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(pbest.p, 0, np * 8, nullptr));
    VSA_HIP(hipMemsetAsync(cbest.p, 0, n * 8, nullptr));
    VSA_HIP(hipMemsetAsync(ctaker.p, 0xFF, n * 4, nullptr));
    VSA_HIP(hipMemsetAsync(kth.p, 0, np * 8, nullptr));
    k_ch_pid<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(pstart.as<uint64_t>(), np,
                                                   n, pid.as<uint32_t>());
    VSA_HIP(hipGetLastError());
    const Retr q = {c->params,
                    fr,
                    pstart.as<uint64_t>(),
                    pid.as<uint32_t>(),
                    n,
                    rm.as<uint8_t>(),
                    pbest.as<unsigned long long>(),
                    cbest.as<unsigned long long>(),
                    ctaker.as<uint32_t>(),
                    kth.as<int64_t>(),
                    thr.as<int64_t>()};
    k_ch_ends<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(q);
    VSA_HIP(hipGetLastError());
    if (c->params.kind == VSA_CHAIN_LOCAL_BEST)
    {
      k_ch_kth<<<vsa_grid((np + TC_BLOCK / 64 - 1) / (TC_BLOCK / 64)),
                 TC_BLOCK, 0, nullptr>>>(q, np);
      VSA_HIP(hipGetLastError());
    }
    k_ch_threshold<<<gridfor(np), TC_BLOCK, 0, nullptr>>>(q, np);
    VSA_HIP(hipGetLastError());
    if (vsa_ch_islocal(c->params.kind))
    {
      k_ch_takers<<<gridfor(n), TC_BLOCK, 0, nullptr>>>(q);
      VSA_HIP(hipGetLastError());
    }
    EndF ef = {q, nullptr};
    uint64_t nchains = 0, chained = 0;
    if (tc_count<1, 1>(ef, n, eoff, &nchains) != 0)
    {
      return -100;
    }
    if (nchains > 0)
    {
      DevBuf cproblem, cnumber, cscore, clength, cstart;
      if (ends.alloc(nchains * 4) != 0 || cproblem.alloc(nchains * 8) != 0 ||
          cnumber.alloc(nchains * 8) != 0 || cscore.alloc(nchains * 8) != 0 ||
          clength.alloc((nchains + 1) * 8) != 0 ||
          cstart.alloc((nchains + 1) * 8) != 0)
      {
        return -100;
      }
      ef.ends = ends.as<uint32_t>();
      if (tc_emit<1>(ef, n, eoff) != 0)
      {
        return -100;
      }
      k_ch_chains<<<gridfor(nchains + 1), TC_BLOCK, 0, nullptr>>>(
          q, ends.as<uint32_t>(), nchains, cproblem.as<uint64_t>(),
          cnumber.as<uint64_t>(), cscore.as<int64_t>(),
          clength.as<uint64_t>());
      VSA_HIP(hipGetLastError());
      if (exclusive_sum(clength.as<uint64_t>(), cstart.as<uint64_t>(), nchains,
                        nullptr, &chained) != 0 ||
          members.alloc(chained * 4) != 0)
      {
        return -100;
      }
      k_ch_members<<<gridfor(nchains), TC_BLOCK, 0, nullptr>>>(
          q, ends.as<uint32_t>(), nchains, cstart.as<uint64_t>(),
          srt.idx.as<uint32_t>(), members.as<uint32_t>());
      VSA_HIP(hipGetLastError());
      hproblem.resize(nchains);
      hnumber.resize(nchains);
      hscore.resize(nchains);
      hstart.resize(nchains + 1);
      VSA_HIP(hipMemcpy(hproblem.data(), cproblem.p, nchains * 8,
                        hipMemcpyDeviceToHost));
      VSA_HIP(hipMemcpy(hnumber.data(), cnumber.p, nchains * 8,
                        hipMemcpyDeviceToHost));
      VSA_HIP(hipMemcpy(hscore.data(), cscore.p, nchains * 8,
                        hipMemcpyDeviceToHost));
      VSA_HIP(hipMemcpy(hstart.data(), cstart.p, (nchains + 1) * 8,
                        hipMemcpyDeviceToHost));
    }
    tretr.stop();
    VSA_HIP(hipStreamSynchronize(nullptr));
    st.chains = nchains;
    st.chained = chained;
    ms[CH_SORT] = tsort.ms();
    ms[CH_REPLAY] = treplay.ms();
    ms[CH_SCORE] = tscore.ms();
    ms[CH_RETRIEVE] = tretr.ms();
  }
  // from here on nothing fails: the state changes
  vsa_dev_free(c->members);
  c->members = (uint32_t *) members.release();
  c->problem.swap(hproblem);
  c->number.swap(hnumber);
  c->score.swap(hscore);
  c->start.swap(hstart);
  c->stats = st;
  for (int q = 0; q < VSA_CHAIN_STAGES; q++)
  {
    c->ms[q] += ms[q];
  }
  c->finished = c->everfinished = true;
  c->nfinished = c->list.n;
  c->gathered = false;
  return 0;
}

extern "C" int vsa_chain_getstats(const vsa_chain *c, vsa_chainstats *stats)
{
  if (c == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_chain_getstats: NULL argument");
    return -1;
  }
  *stats = c->stats;
  return 0;
}

extern "C" int vsa_chain_chains(const vsa_chain *c, uint64_t *problem,
                                uint64_t *number, int64_t *score,
                                uint64_t *start)
{
  const int rc = needfinished(c, "vsa_chain_chains");
  if (rc != 0)
  {
    return rc;
  }
  const uint64_t k = c->stats.chains;
  if (problem != nullptr && k > 0)
  {
    memcpy(problem, c->problem.data(), k * 8);
  }
  if (number != nullptr && k > 0)
  {
    memcpy(number, c->number.data(), k * 8);
  }
  if (score != nullptr && k > 0)
  {
    memcpy(score, c->score.data(), k * 8);
  }
  if (start != nullptr)
  {
    memcpy(start, c->start.data(), (k + 1) * 8);
  }
  return 0;
}

extern "C" int vsa_chain_members(vsa_chain *c, uint64_t *members)
{
  const int rc = needfinished(c, "vsa_chain_members");
  if (rc != 0)
  {
    return rc;
  }
  if (members == nullptr)
  {
    VSA_ERROR("vsa_chain_members: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0 || hostmembers(c) != 0)
  {
    return -100;
  }
  if (c->stats.chained > 0)
  {
    memcpy(members, c->hmembers.data(), c->stats.chained * 8);
  }
  return 0;
}

extern "C" int vsa_chain_records(vsa_chain *c, vsa_result **records,
                                 uint8_t *palindromic)
{
  const int rc = needfinished(c, "vsa_chain_records");
  if (rc != 0)
  {
    return rc;
  }
  if (records == nullptr)
  {
    VSA_ERROR("vsa_chain_records: NULL argument");
    return -1;
  }
  *records = nullptr;
  if (enter(c->device) != 0)
  {
    return -100;
  }
  return records_of(c->list, c->members, c->stats.chained, palindromic,
                    nullptr, records);
}

extern "C" int64_t vsa_chain_format(vsa_chain *c, vsa_sink *sink, int flags,
                                    char *buffer, uint64_t capacity)
{
  const int rc = needfinished(c, "vsa_chain_format");
  if (rc != 0)
  {
    return rc;
  }
  if (sink == nullptr || buffer == nullptr)
  {
    VSA_ERROR("vsa_chain_format: NULL argument");
    return -1;
  }
  if (enter(c->device) != 0 || hostmembers(c) != 0)
  {
    return -100;
  }
  return vsa_chain_format_host(sink, flags, c->stats.chains, c->number.data(),
                               c->score.data(), c->start.data(),
                               c->memberrecs.data(), buffer, capacity);
}

extern "C" int vsa_chain_times(const vsa_chain *c, double *ms)
{
  if (c == nullptr || ms == nullptr)
  {
    VSA_ERROR("vsa_chain_times: NULL argument");
    return -1;
  }
  memcpy(ms, c->ms, sizeof c->ms);
  return 0;
}
