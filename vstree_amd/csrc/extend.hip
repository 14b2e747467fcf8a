// Degenerate matches, vmatch -l L -h K [-seedlength S] [-q Q] IDX: every
// exact seed of a list that stays in HBM extended to the left and right over
// at most K mismatches (hammingextend, kurtz/extendHD.c:166-374).  The rules
// are extend_rules.h's, which extend_host.c reads too; here is how the
// symbols are read.
//
//   scan    k_ext_scan: one lane per (seed, side).  The border branches of
//           the rules, then both texts in words of 8 bytes from unaligned
//           starts (a left scan reads downwards and swaps the bytes); the
//           marks of a word -- mismatch, wildcard, separator -- become the
//           events of the rules, which write the look table of the side
//           (entry h of item i at look[h * items + i], 32 bits).  A lane that
//           has looked at `budget` symbols without an end puts its item on
//           the long list.
//   long    k_ext_long: one wavefront per item of the long list, from the
//           start of the side: per step 64 lanes x 16 bytes of both texts, a
//           ballot of the lanes that hold a mark, and the marks of those
//           lanes in order through the same events, so that the (K+1)-th
//           mismatch, the first separator and the left stop rule fall where
//           the lane scan would put them.  The grid is fixed; the wavefronts
//           take items until the count the scan stage left is reached, so
//           the host does not wait between the stages.
//   choice  k_ext_choose: one lane per seed, the O(K^2) loop of the rules on
//           the E-value table, the match record and a keep flag.
//   compact the shared stable compaction (tile_compact.inc): the matches in
//           the order of their seeds.
// Nothing is read through a seed that does not fit its texts: such a seed is
// counted and the call fails.
#define VSA_EXT_LOOK uint32_t
#include "search_host.hpp"
#include "tile_compact.inc"
#include "extend_rules.h"

namespace
{

#define EXT_MISFIT 0xFFFFFFFFu
#define EXT_BLOCK 256
// the driver, the word load and the words of the counters; EXT_NSTAGE
// counts the items on the long list
#include "extend_shared.hpp"

struct ExtParams
{
  const uint8_t *tis;
  uint64_t n;
  DevQueries q;
  int self;
  const vsa_match *seeds;
  uint64_t nseeds, nitems;
  uint64_t leastlength, seedlength;
  uint32_t maxdist, budget;
  uint32_t *look; // [(maxdist + 1) * nitems]
  uint32_t *hout; // [nitems]: mismatches the side offers, or EXT_MISFIT
  uint32_t *longlist;
  unsigned long long *counters;
};

// the two views of a seed and its place in the second; false: it does not fit
__device__ __forceinline__ bool ext_views(const ExtParams &p,
                                          const vsa_match &m,
                                          vsa_ext_view &v1, vsa_ext_view &v2,
                                          uint64_t &pos2)
{
  v1.p = p.tis;
  v1.len = p.n;
  v1.atstart = v1.atend = 1;
  if (m.length == 0 || m.dbstart > p.n || m.length > p.n - m.dbstart)
  {
    return false;
  }
  if (p.self)
  {
    v2 = v1;
    pos2 = m.queryseq;
    return pos2 <= p.n && m.length <= p.n - pos2;
  }
  const uint64_t q = m.queryseq - p.q.seqoffset;
  if (m.queryseq < p.q.seqoffset || q >= p.q.nq)
  {
    return false;
  }
  const uint64_t qlen = p.q.uniformlen != 0 ? p.q.uniformlen : p.q.length[q],
                 qstart = p.q.dense ? q * p.q.uniformlen : p.q.start[q];
  v2.p = p.q.symbols + qstart;
  v2.len = qlen;
  v2.atstart = q == 0;
  v2.atend = q + 1 == p.q.nq;
  pos2 = m.querystart;
  return pos2 <= qlen && m.length <= qlen - pos2;
}

// sixteen symbols at t0 .. t0 + 15 as two such words
__device__ __forceinline__ void ext_word16(const uint8_t *p, int left,
                                           uint64_t t0, uint64_t valid,
                                           uint64_t &w0, uint64_t &w1)
{
  if (valid < 16)
  {
    w0 = vsa_ext_word(p, left, t0, valid);
    w1 = vsa_ext_word(p, left, t0 + 8, valid > 8 ? valid - 8 : 0);
    return;
  }
  if (left)
  {
    const vsa_u128 v = vsa_load16(p - t0 - 15);
    w0 = __builtin_bswap64(v.hi);
    w1 = __builtin_bswap64(v.lo);
  } else
  {
    const vsa_u128 v = vsa_load16(p + t0);
    w0 = v.lo;
    w1 = v.hi;
  }
}

__global__ void __launch_bounds__(EXT_BLOCK) k_ext_scan(ExtParams p)
{
  const uint64_t item = vsa_bid() * EXT_BLOCK + threadIdx.x;
  bool tolong = false;

  if (item < p.nitems)
  {
    const vsa_match m = p.seeds[item >> 1];
    const int left = (item & 1) == 0;
    vsa_ext_view v1, v2;
    uint64_t pos2;

    if (!ext_views(p, m, v1, v2, pos2))
    {
      p.hout[item] = EXT_MISFIT;
    } else
    {
      vsa_ext_scan s;
      vsa_ext_plan plan;
      uint32_t h = 0;

      vsa_ext_begin(&s, p.look + item, p.nitems, p.maxdist, p.seedlength,
                    left);
      if (vsa_ext_prepare(&s, &v1, m.dbstart, &v2, pos2, m.length, &plan,
                          &h) == VSA_EXT_SCAN)
      {
        uint64_t t0 = 0;
        bool over = false;
        while (!over && t0 < plan.nsym && t0 < p.budget)
        {
          uint32_t sep;
          const uint64_t a = ext_word(plan.p1, left, t0, plan.nsym - t0),
                         b = ext_word(plan.p2, left, t0, plan.nsym - t0);
          const uint32_t marks = vsa_ext_marks8(a, b, &sep);
          over = vsa_ext_events(&s, &plan, t0, marks, sep) != 0;
          t0 += 8;
        }
        if (!over && t0 < plan.nsym)
        {
          tolong = true;
        } else
        {
          if (!over)
          {
            (void) vsa_ext_finish(&s, &plan);
          }
          h = vsa_ext_end(&s);
        }
      }
      if (!tolong)
      {
        p.hout[item] = h;
      }
    }
  }
  const uint64_t slot = vsa_wave_reserve01(p.counters + EXT_NSTAGE, tolong);
  if (tolong)
  {
    p.longlist[slot] = (uint32_t) item;
  }
}

__global__ void __launch_bounds__(EXT_BLOCK) k_ext_long(ExtParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = vsa_nblocks() * (EXT_BLOCK / 64),
                 nlong = p.counters[EXT_NSTAGE];

  for (uint64_t w = vsa_bid() * (EXT_BLOCK / 64) + (threadIdx.x >> 6);
       w < nlong; w += nwaves)
  {
    const uint32_t item = p.longlist[w];
    const vsa_match m = p.seeds[item >> 1];
    const int left = (item & 1u) == 0;
    vsa_ext_view v1, v2;
    vsa_ext_scan s;
    vsa_ext_plan plan;
    uint64_t pos2;
    uint32_t h = 0;

    // (the scan stage has seen that the seed fits and that the side is one
    // to scan; every lane keeps the state, lane 0 writes the table)
    if (!ext_views(p, m, v1, v2, pos2))
    {
      continue;
    }
    vsa_ext_begin(&s, lane == 0 ? p.look + item : nullptr, p.nitems,
                  p.maxdist, p.seedlength, left);
    if (vsa_ext_prepare(&s, &v1, m.dbstart, &v2, pos2, m.length, &plan, &h) !=
        VSA_EXT_SCAN)
    {
      continue;
    }
    bool over = false;
    for (uint64_t t0 = 0; !over; t0 += VSA_EXTEND_LONG_STEP)
    {
      const uint64_t base = t0 + 16u * lane;
      const uint64_t valid =
          base < plan.nsym ? (plan.nsym - base < 16 ? plan.nsym - base : 16)
                           : 0;
      uint32_t marks = 0, seps = 0;
      if (valid > 0)
      {
        uint64_t a0, a1, b0, b1;
        uint32_t s0, s1;
        ext_word16(plan.p1, left, base, valid, a0, a1);
        ext_word16(plan.p2, left, base, valid, b0, b1);
        marks = vsa_ext_marks8(a0, b0, &s0);
        marks |= vsa_ext_marks8(a1, b1, &s1) << 8;
        seps = s0 | s1 << 8;
        marks &= (1u << valid) - 1u;
      }
      // the lanes that hold a mark, in the order of the symbols
      unsigned long long any = __ballot(marks != 0);
      while (any != 0 && !over)
      {
        const int l = __ffsll(any) - 1;
        any &= any - 1;
        const uint32_t lm = __shfl(marks, l, 64), ls = __shfl(seps, l, 64);
        over = vsa_ext_events(&s, &plan, t0 + 16u * (uint32_t) l, lm, ls) != 0;
      }
      if (!over && t0 + VSA_EXTEND_LONG_STEP >= plan.nsym)
      {
        over = vsa_ext_finish(&s, &plan) != 0;
      }
    }
    if (lane == 0)
    {
      p.hout[item] = vsa_ext_end(&s);
    }
  }
}

__global__ void __launch_bounds__(EXT_BLOCK)
k_ext_choose(ExtParams p, vsa_selrules ev, vsa_match *__restrict__ out,
             uint8_t *__restrict__ keep)
{
  const uint64_t i = vsa_bid() * EXT_BLOCK + threadIdx.x;
  bool misfit = false;
  uint64_t len = 0;

  if (i < p.nseeds)
  {
    const uint32_t hleft = p.hout[2 * i], hright = p.hout[2 * i + 1];
    uint8_t k = 0;
    if (hleft == EXT_MISFIT || hright == EXT_MISFIT)
    {
      misfit = true;
    } else
    {
      const vsa_match m = p.seeds[i];
      uint64_t shift = 0, dist = 0;
      if (vsa_ext_choose(&ev, m.length, p.leastlength, p.maxdist,
                         p.look + 2 * i, hleft, p.look + 2 * i + 1, hright,
                         p.nitems, &shift, &len, &dist))
      {
        vsa_match o;
        o.length = VSA_HAMMING_PACK(len, dist);
        o.dbstart = m.dbstart - shift;
        o.queryseq = p.self ? m.queryseq - shift : m.queryseq;
        o.querystart = p.self ? 0 : m.querystart - shift;
        out[i] = o;
        k = 1;
      } else
      {
        len = 0;
      }
    }
    keep[i] = k;
  }
  // one atomic per wavefront for each of the two counts (stated in both
  // choice kernels: as a shared inline function the sum below came out with
  // the operands of one addition swapped in the device listing)
  const unsigned long long bad = __ballot(misfit);
  uint64_t sum = len;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    sum += vsa_shfl64(sum, (int) ((threadIdx.x & 63u) ^ (uint32_t) d));
  }
  if ((threadIdx.x & 63u) == 0)
  {
    if (bad != 0)
    {
      atomicAdd(p.counters + EXT_NMISFIT, (unsigned long long) __popcll(bad));
    }
    if (sum != 0)
    {
      atomicAdd(p.counters + EXT_SUMLENGTH, (unsigned long long) sum);
    }
  }
}

// what the driver of extend_shared.hpp is given
struct Hamming
{
  static constexpr uint32_t cap = VSA_EXTEND_MAXDIST;
  static constexpr bool evalues = true, hequot = false;
  static void hosttakes(char *buf, size_t n)
  {
    snprintf(buf, n, "vsa_extend_hamming_host takes any");
  }
  static int checkbound(const char *who, uint64_t maxdist)
  {
    return capbound<Hamming>(who, maxdist);
  }
  static uint64_t seedlength(uint64_t leastlength, uint64_t maxdist,
                             uint64_t seedlength)
  {
    return vsa_ext_seedlength(leastlength, maxdist, seedlength);
  }

  struct Stage
  {
    // (the timers first: what is made behind a member whose constructor may
    // throw is destroyed out of line, and DevBuf's destructor would become a
    // symbol of the library)
    Timer tscan{nullptr}, tlong{nullptr};
    ExtParams p;
    DevBuf look, hout, longlist;

    int prepare(const ExtCall &c, Timer &)
    {
      memset(&p, 0, sizeof p);
      p.tis = c.index->tis_alloc + VSA_TIS_FRONTPAD;
      p.n = c.index->n;
      p.self = c.self;
      if (!c.self)
      {
        p.q = devqueries(c.queries);
      }
      p.seeds = c.seeds->matches;
      p.nseeds = c.seeds->count;
      p.nitems = 2 * c.seeds->count;
      p.leastlength = c.leastlength;
      p.seedlength = c.seedlength;
      p.maxdist = (uint32_t) c.maxdist;
      p.budget = lanebudget();
      if (look.alloc((c.maxdist + 1) * p.nitems * 4) != 0 ||
          hout.alloc(p.nitems * 4) != 0 || longlist.alloc(p.nitems * 4) != 0)
      {
        return -100;
      }
      p.look = look.as<uint32_t>();
      p.hout = hout.as<uint32_t>();
      p.longlist = longlist.as<uint32_t>();
      return 0;
    }

    int run(const ExtCall &c, vsa_match *recs, uint8_t *keep,
            unsigned long long *counters, Timer &tall, Timer &tsearch)
    {
      p.counters = counters;
      tall.start();
      VSA_HIP(hipMemsetAsync(counters, 0, EXT_NCOUNTERS * 8, nullptr));
      tsearch.start();
      tscan.start();
      k_ext_scan<<<vsa_grid((p.nitems + EXT_BLOCK - 1) / EXT_BLOCK),
                   EXT_BLOCK, 0, nullptr>>>(p);
      VSA_HIP(hipGetLastError());
      tscan.stop();
      // (a wavefront per item at most, and no more than fill the device a
      // few times over: the wavefronts take items until the list is done)
      const uint64_t longblocks = std::min<uint64_t>(
          (p.nitems + EXT_BLOCK / 64 - 1) / (EXT_BLOCK / 64), 8192);
      tlong.start();
      k_ext_long<<<vsa_grid(longblocks), EXT_BLOCK, 0, nullptr>>>(p);
      VSA_HIP(hipGetLastError());
      tlong.stop();
      k_ext_choose<<<vsa_grid((p.nseeds + EXT_BLOCK - 1) / EXT_BLOCK),
                     EXT_BLOCK, 0, nullptr>>>(p, c.ev, recs, keep);
      VSA_HIP(hipGetLastError());
      tsearch.stop();
      return 0;
    }

    void stats(vsa_stats &st)
    {
      st.first_kernel_ms = tscan.ms();
      st.anchor_ms = tlong.ms();
    }
  };
};

} // namespace

extern "C" uint32_t vsa_extend_maxdist(void)
{
  return VSA_EXTEND_MAXDIST;
}

extern "C" uint32_t vsa_extend_lane_budget(void)
{
  return VSA_EXTEND_LANE_BUDGET;
}

extern "C" uint32_t vsa_extend_long_step(void)
{
  return VSA_EXTEND_LONG_STEP;
}

extern "C" uint64_t vsa_extend_seedlength(uint64_t leastlength,
                                          uint64_t maxdist,
                                          uint64_t seedlength)
{
  return vsa_ext_seedlength(leastlength, maxdist, seedlength);
}

extern "C" int vsa_extend_hamming(const vsa_index *index,
                                  const vsa_queries *queries,
                                  const vsa_result *seeds,
                                  const vsa_sinkparams *layout,
                                  int palindromic, uint64_t leastlength,
                                  uint64_t maxdist, uint64_t seedlength,
                                  vsa_result **result)
{
  return extend_list<Hamming>("vsa_extend_hamming", index, queries, seeds,
                              layout, palindromic, leastlength, maxdist,
                              seedlength, result);
}

extern "C" int vsa_findquerymatches_hamming(const vsa_index *index,
                                            const vsa_queries *queries,
                                            uint64_t leastlength,
                                            uint64_t maxdist,
                                            uint64_t seedlength,
                                            int palindromic,
                                            vsa_result **result)
{
  return extend_queries<Hamming>("vsa_findquerymatches_hamming", index,
                                 queries, leastlength, maxdist, seedlength,
                                 palindromic, result);
}

extern "C" int vsa_findselfmatches_hamming(const vsa_index *index,
                                           uint64_t leastlength,
                                           uint64_t maxdist,
                                           uint64_t seedlength,
                                           vsa_result **result)
{
  return extend_self<Hamming>("vsa_findselfmatches_hamming", index,
                              leastlength, maxdist, seedlength, result);
}
