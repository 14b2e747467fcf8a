// Degenerate matches by edit distance, vmatch -l L -e K [-seedlength S] [-p]
// [-q Q] IDX: every exact seed of a list that stays in HBM extended to the
// left and right over at most K edit operations (editextend,
// kurtz/extendED.c:78-355).  The rules are extend_edist_rules.h's, which
// extend_edist_host.c reads too; here is how the fronts are made.
//
//   flatten k_flatten (extend_flat.hpp): the query batch as the reference's
//           Multiseq, one array with a separator between two sequences (the
//           rules say why the fronts need it), one wavefront per sequence.
//   fronts  k_ed_fronts<W>: one group of W = 16, 32 or 64 lanes per (seed,
//           side), chosen by 2 K + 1; lane l is the diagonal l - K.  Per
//           front: the rows of the neighbouring diagonals by shuffles, the
//           entry of the rules, the slide along both texts in words of 8
//           bytes from unaligned starts (a left side reads downwards and
//           swaps the bytes; the last partial word byte by byte).  A slide
//           that has not ended after `budget` symbols is finished by the
//           group together: every lane takes one word of the stretch, a
//           ballot finds the first mark.  The lanes slide at once under the
//           bounds of the start of the front; if one of them read a
//           separator, the slides are replayed in ascending order of the
//           diagonals (vsa_ed_replay), so that every diagonal gets the bounds
//           the reference's order shows it.  Every front goes to scratch as
//           it is finished, entry (p, k) of item i at
//           fronts[i * (K + 1)^2 + p^2 + k + p]: the lanes of a group write
//           neighbouring words.
//   choice  k_ed_choose: one lane per seed, the loop of the rules over the
//           stored fronts on the E-value table, the match record and a keep
//           flag.
//   compact the shared stable compaction (tile_compact.inc): the matches in
//           the order of their seeds.
// The seed list is worked through in pieces whose fronts fit a fixed scratch
// budget.  Nothing is read through a seed that does not fit its texts: such
// a seed is counted and the call fails.
#define VSA_ED_ROW uint32_t
#include "search_host.hpp"
#include "tile_compact.inc"
#include "extend_edist_rules.h"

namespace
{

// the driver, the word load and the words of the counters; EXT_NSTAGE
// counts the sides with a slide the group finished, EXT_SUMLENGTH sums
// length1 of the matches
#include "extend_shared.hpp"
// the query Multiseq (k_flatten)
#include "extend_flat.hpp"

#define ED_MISFIT 0xFFFFFFFFu
#define ED_BLOCK 256
// device scratch of the fronts of one piece of the seed list
#define ED_SCRATCH ((uint64_t) 256 << 20)

static_assert(2 * VSA_EXTEND_EDIST_MAXDIST + 1 <= 64,
              "the diagonals of a front are the lanes of one wavefront");

struct EdParams
{
  const uint8_t *s1, *s2; // the two Multiseqs
  uint64_t n1, n2;
  DevQueries q;
  const uint64_t *abs2; // ragged batches: where the sequences begin in s2
  int self;
  const vsa_match *seeds;
  uint64_t first, count; // the piece of the seed list
  uint64_t leastlength, seedlength;
  uint32_t maxdist, budget;
  uint32_t *fronts; // [2 * count * (maxdist + 1)^2]
  uint32_t *hout;   // [2 * count]: the last front of the side, or ED_MISFIT
  unsigned long long *counters;
};

// the place of a seed in the second Multiseq; false: it does not fit
__device__ __forceinline__ bool ed_place(const EdParams &p, const vsa_match &m,
                                         uint64_t &pos2)
{
  if (m.length == 0 || m.dbstart > p.n1 || m.length > p.n1 - m.dbstart)
  {
    return false;
  }
  if (p.self)
  {
    pos2 = m.queryseq;
    return pos2 <= p.n1 && m.length <= p.n1 - pos2;
  }
  const uint64_t q = m.queryseq - p.q.seqoffset;
  if (m.queryseq < p.q.seqoffset || q >= p.q.nq)
  {
    return false;
  }
  const uint64_t qlen = flat_qlength(p, q);
  pos2 = flat_qabs(p, q) + m.querystart;
  return m.querystart <= qlen && m.length <= qlen - m.querystart;
}

// the marks of the words at offset `at` of a slide from (t, t + k) of which
// `valid` symbols are below the bounds; a, c: the words
__device__ __forceinline__ uint32_t ed_marks(const vsa_ed_side &s, int64_t t,
                                             int64_t k, int64_t at,
                                             int64_t valid, uint64_t &a,
                                             uint64_t &c)
{
  const uint8_t *pu = s.s1 + (s.left ? s.o1 - t : s.o1 + t),
                *pv = s.s2 + (s.left ? s.o2 - (t + k) : s.o2 + (t + k));
  uint32_t sep;

  a = ext_word(pu, s.left, (uint64_t) at, (uint64_t) valid);
  c = ext_word(pv, s.left, (uint64_t) at, (uint64_t) valid);
  const uint32_t marks = vsa_ext_marks8(a, c, &sep);
  return valid < 8 ? marks & ((1u << valid) - 1u) : marks;
}

__device__ __forceinline__ int64_t ed_shfl64(int64_t v, int src, int width)
{
  const int lo = __shfl((int) (uint32_t) (uint64_t) v, src, width),
            hi = __shfl((int) (uint32_t) ((uint64_t) v >> 32), src, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

__device__ __forceinline__ int64_t ed_shfl64_up(int64_t v, int width)
{
  const int lo = __shfl_up((int) (uint32_t) (uint64_t) v, 1, width),
            hi = __shfl_up((int) (uint32_t) ((uint64_t) v >> 32), 1, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

__device__ __forceinline__ int64_t ed_shfl64_down(int64_t v, int width)
{
  const int lo = __shfl_down((int) (uint32_t) (uint64_t) v, 1, width),
            hi = __shfl_down((int) (uint32_t) ((uint64_t) v >> 32), 1, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

// Every ballot and shuffle below is executed by all lanes of the wavefront:
// the loops run while ANY group of the wavefront has work, and a group
// without work goes through them with nothing to do.
template <int W>
__global__ void __launch_bounds__(ED_BLOCK) k_ed_fronts(EdParams p)
{
  static_assert(W == 16 || W == 32 || W == 64, "a group divides a wavefront");
  const uint64_t g = (vsa_bid() * ED_BLOCK + threadIdx.x) / W;
  const int gl = (int) (threadIdx.x % W);
  // the bits of this group in a ballot
  const uint32_t shift = (threadIdx.x & 63u) & ~(uint32_t) (W - 1);
  const uint64_t groupbits = W == 64 ? ~(uint64_t) 0
                                     : (((uint64_t) 1 << (W & 63)) - 1);
  const uint64_t words = vsa_ed_frontwords(p.maxdist);
  const int64_t k = (int64_t) gl - (int64_t) p.maxdist;
  bool active = g < 2 * p.count, coop = false;
  vsa_ed_side s;
  vsa_ed_bounds b;
  uint32_t *fr = nullptr;
  int64_t row = 0;
  int foundseed = 0;

  memset(&s, 0, sizeof s);
  b.ub = b.vb = 0;
  if (active)
  {
    const vsa_match m = p.seeds[p.first + (g >> 1)];
    uint64_t pos2 = 0;
    if (!ed_place(p, m, pos2))
    {
      active = false;
      if (gl == 0)
      {
        p.hout[g] = ED_MISFIT;
      }
    } else
    {
      vsa_ed_side_init(&s, p.s1, p.n1, p.s2, p.n2, p.self, m.dbstart, pos2,
                       m.length, (g & 1) == 0, p.maxdist, p.seedlength);
      vsa_ed_bounds_init(&s, &b);
      fr = p.fronts + g * words;
      row = k == 0 ? 0 : s.neg;
      if (k == 0)
      {
        fr[0] = 0;
      }
      if (vsa_ed_bothempty(&s))
      {
        active = false;
        if (gl == 0)
        {
          p.hout[g] = 0;
        }
      }
    }
  }
  for (int64_t pth = 1; __ballot(active) != 0; pth++)
  {
    int64_t below = ed_shfl64_up(row, W), above = ed_shfl64_down(row, W);
    int64_t t = 0, mlen = 0, rem = 0;
    int kind = VSA_ED_NONE, read = 0, seps = 0;
    bool unfinished = false;

    if (active)
    {
      if (gl == 0)
      {
        below = s.neg;
      }
      if (gl == W - 1)
      {
        above = s.neg;
      }
      if (k <= (int64_t) p.maxdist && vsa_ed_evaluated(&s, pth, k))
      {
        kind = vsa_ed_start(&s, row, below, above, k, &t);
      }
      if (kind == VSA_ED_SLIDE)
      {
        const int64_t ru = b.ub - t, rv = b.vb - (t + k);
        rem = ru < rv ? ru : rv;
        rem = rem < 0 ? 0 : rem;
        bool done = rem == 0;
        while (!done && mlen < (int64_t) p.budget)
        {
          uint64_t a, c;
          const int64_t valid = rem - mlen;
          const uint32_t marks = ed_marks(s, t, k, mlen, valid, a, c);
          if (marks != 0)
          {
            const uint32_t j = (uint32_t) __builtin_ctz(marks);
            seps = vsa_ed_seps(a, c, j);
            mlen += j;
            read = 1;
            done = true;
          } else
          {
            mlen += valid < 8 ? valid : 8;
            done = mlen >= rem;
          }
        }
        unfinished = !done;
      }
    }
    // the slides that are over the budget, one after the other, by the group
    while (__ballot(unfinished) != 0)
    {
      const uint64_t todo = (__ballot(unfinished) >> shift) & groupbits;
      const int j = todo != 0 ? __ffsll((unsigned long long) todo) - 1 : 0;
      const int64_t jt = ed_shfl64(t, j, W), jm = ed_shfl64(mlen, j, W),
                    jrem = ed_shfl64(rem, j, W),
                    jk = (int64_t) j - (int64_t) p.maxdist;
      const int64_t at = jm + 8 * (int64_t) gl;
      uint32_t marks = 0, first = 0;
      int myseps = 0;
      if (todo != 0 && at < jrem)
      {
        uint64_t a, c;
        marks = ed_marks(s, jt, jk, at, jrem - at, a, c);
        if (marks != 0)
        {
          first = (uint32_t) __builtin_ctz(marks);
          myseps = vsa_ed_seps(a, c, first);
        }
      }
      const uint64_t hit = (__ballot(marks != 0) >> shift) & groupbits;
      const int f = hit != 0 ? __ffsll((unsigned long long) hit) - 1 : 0;
      const uint32_t ffirst = (uint32_t) __shfl((int) first, f, W);
      const int fseps = __shfl(myseps, f, W);
      if (todo != 0)
      {
        coop = true;
        if (gl == j)
        {
          if (hit != 0)
          {
            mlen = jm + 8 * (int64_t) f + (int64_t) ffirst;
            read = 1;
            seps = fseps;
            unfinished = false;
          } else if (jm + 8 * W >= jrem)
          {
            mlen = jrem;
            unfinished = false;
          } else
          {
            mlen = jm + 8 * W;
          }
        }
      }
    }
    // a separator was read: the bounds in the order of the diagonals
    vsa_ed_bounds mine = b;
    if (__ballot(active && read && seps != 0) != 0)
    {
      vsa_ed_bounds run = b;
      const int packed = kind | read << 2 | seps << 3;
      for (int j = 0; j < W; j++)
      {
        const int jp = __shfl(packed, j, W);
        const int64_t jt = ed_shfl64(t, j, W), jm = ed_shfl64(mlen, j, W);
        int64_t m2 = jm;
        if ((jp & 3) == VSA_ED_SLIDE)
        {
          m2 = vsa_ed_replay(jt, (int64_t) j - (int64_t) p.maxdist, jm,
                             jp >> 2 & 1, jp >> 3, &run);
        }
        if (gl == j)
        {
          mlen = m2;
          mine = run;
        }
      }
      b = run;
    }
    int found = 0;
    int64_t value = 0;
    if (active)
    {
      value = vsa_ed_stored(&s, kind, t, mlen, k, &mine, &found);
    }
    const bool anyfound =
        ((__ballot(active && found != 0) >> shift) & groupbits) != 0;
    const bool defined =
        ((__ballot(active && value >= 0) >> shift) & groupbits) != 0;
    if (active)
    {
      uint32_t h = 0;
      foundseed |= anyfound ? 1 : 0;
      row = value;
      if (k >= -pth && k <= pth)
      {
        fr[vsa_ed_at(pth, k)] = value < 0 ? VSA_ED_UNDEF : (uint32_t) value;
      }
      if (vsa_ed_frontends(&s, pth, defined, foundseed, &h))
      {
        active = false;
        if (gl == 0)
        {
          p.hout[g] = h;
        }
      }
    }
  }
  if (coop && gl == 0)
  {
    atomicAdd(p.counters + EXT_NSTAGE, 1ull);
  }
}

__global__ void __launch_bounds__(ED_BLOCK)
k_ed_choose(EdParams p, vsa_selrules ev, vsa_match *__restrict__ out,
            uint8_t *__restrict__ keep)
{
  const uint64_t i = vsa_bid() * ED_BLOCK + threadIdx.x;
  bool misfit = false;
  uint64_t len = 0;

  if (i < p.count)
  {
    const uint32_t hleft = p.hout[2 * i], hright = p.hout[2 * i + 1];
    const vsa_match m = p.seeds[p.first + i];
    uint64_t pos2 = 0;
    uint8_t kept = 0;
    if (hleft == ED_MISFIT || hright == ED_MISFIT || !ed_place(p, m, pos2))
    {
      misfit = true;
    } else
    {
      const uint64_t words = vsa_ed_frontwords(p.maxdist);
      vsa_ed_side ls, rs;
      vsa_ed_match best;
      vsa_ed_side_init(&ls, p.s1, p.n1, p.s2, p.n2, p.self, m.dbstart, pos2,
                       m.length, 1, p.maxdist, p.seedlength);
      vsa_ed_side_init(&rs, p.s1, p.n1, p.s2, p.n2, p.self, m.dbstart, pos2,
                       m.length, 0, p.maxdist, p.seedlength);
      if (vsa_ed_choose(&ev, &ls, &rs, p.self, m.dbstart, pos2, m.length,
                        p.leastlength, p.fronts + 2 * i * words, hleft,
                        p.fronts + (2 * i + 1) * words, hright, &best))
      {
        vsa_match o;
        vsa_ed_record(&m, p.self, pos2, &best, &o);
        out[p.first + i] = o;
        len = best.length1;
        kept = 1;
      }
    }
    keep[p.first + i] = kept;
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

// VSA_EXTEND_EDIST_SCRATCH: bytes of front scratch instead of ED_SCRATCH
uint64_t scratchbudget()
{
  const char *e = getenv("VSA_EXTEND_EDIST_SCRATCH");
  const uint64_t v = e != nullptr ? strtoull(e, nullptr, 10) : 0;
  return v != 0 ? v : ED_SCRATCH;
}

template <int W>
int launchfronts(const EdParams &p)
{
  const uint64_t groups = ED_BLOCK / W;
  k_ed_fronts<W><<<vsa_grid((2 * p.count + groups - 1) / groups), ED_BLOCK, 0,
                   nullptr>>>(p);
  VSA_HIP(hipGetLastError());
  return 0;
}

// what the driver of extend_shared.hpp is given
struct Edist
{
  static constexpr uint32_t cap = VSA_EXTEND_EDIST_MAXDIST;
  static constexpr bool evalues = true, hequot = true;
  static void hosttakes(char *buf, size_t n)
  {
    snprintf(buf, n, "vsa_extend_edist_host takes up to %u",
             VSA_EDIST_MAXDISTANCE);
  }
  static int checkbound(const char *who, uint64_t maxdist)
  {
    return capbound<Edist>(who, maxdist);
  }
  static uint64_t seedlength(uint64_t leastlength, uint64_t maxdist,
                             uint64_t seedlength)
  {
    return vsa_ext_seedlength(leastlength, maxdist, seedlength);
  }

  struct Stage
  {
    EdParams p;
    DevBuf flat, abs2, fronts, hout;
    uint64_t piece = 0;
    float frontsms = 0.0f;

    // the query Multiseq and the fronts of one piece of the seed list
    int prepare(const ExtCall &c, Timer &tall)
    {
      memset(&p, 0, sizeof p);
      p.s1 = c.index->tis_alloc + VSA_TIS_FRONTPAD;
      p.n1 = c.index->n;
      p.self = c.self;
      p.seeds = c.seeds->matches;
      p.leastlength = c.leastlength;
      p.seedlength = c.seedlength;
      p.maxdist = (uint32_t) c.maxdist;
      p.budget = lanebudget();
      tall.start();
      if (c.self)
      {
        p.s2 = p.s1;
        p.n2 = p.n1;
      } else
      {
        const int rc = flatten_batch(c.who, c.queries, p, flat, abs2);
        if (rc != 0)
        {
          return rc;
        }
      }
      const uint64_t words = vsa_ed_frontwords(c.maxdist);
      piece = std::min<uint64_t>(
          c.seeds->count,
          std::max<uint64_t>(scratchbudget() / (2 * words * 4), 1));
      if (fronts.alloc(piece * 2 * words * 4) != 0 ||
          hout.alloc(piece * 2 * 4) != 0)
      {
        return -100;
      }
      p.fronts = fronts.as<uint32_t>();
      p.hout = hout.as<uint32_t>();
      return 0;
    }

    int run(const ExtCall &c, vsa_match *recs, uint8_t *keep,
            unsigned long long *counters, Timer &, Timer &tsearch)
    {
      const uint64_t nseeds = c.seeds->count;
      p.counters = counters;
      VSA_HIP(hipMemsetAsync(counters, 0, EXT_NCOUNTERS * 8, nullptr));
      tsearch.start();
      for (uint64_t first = 0; first < nseeds; first += piece)
      {
        p.first = first;
        p.count = std::min<uint64_t>(piece, nseeds - first);
        Timer tf(nullptr);
        tf.start();
        const int rc = c.maxdist <= 7    ? launchfronts<16>(p)
                       : c.maxdist <= 15 ? launchfronts<32>(p)
                                         : launchfronts<64>(p);
        if (rc != 0)
        {
          return rc;
        }
        tf.stop();
        k_ed_choose<<<vsa_grid((p.count + ED_BLOCK - 1) / ED_BLOCK), ED_BLOCK,
                      0, nullptr>>>(p, c.ev, recs, keep);
        VSA_HIP(hipGetLastError());
        VSA_HIP(hipStreamSynchronize(nullptr));
        frontsms += tf.ms();
      }
      tsearch.stop();
      return 0;
    }

    void stats(vsa_stats &st)
    {
      st.first_kernel_ms = frontsms;
    }
  };
};

} // namespace

extern "C" uint32_t vsa_extend_edist_maxdist(void)
{
  return VSA_EXTEND_EDIST_MAXDIST;
}

extern "C" int vsa_extend_edist(const vsa_index *index,
                                const vsa_queries *queries,
                                const vsa_result *seeds,
                                const vsa_sinkparams *layout, int palindromic,
                                uint64_t leastlength, uint64_t maxdist,
                                uint64_t seedlength, vsa_result **result)
{
  return extend_list<Edist>("vsa_extend_edist", index, queries, seeds, layout,
                            palindromic, leastlength, maxdist, seedlength,
                            result);
}

extern "C" int vsa_findquerymatches_edist(const vsa_index *index,
                                          const vsa_queries *queries,
                                          uint64_t leastlength,
                                          uint64_t maxdist,
                                          uint64_t seedlength,
                                          int palindromic,
                                          vsa_result **result)
{
  return extend_queries<Edist>("vsa_findquerymatches_edist", index, queries,
                               leastlength, maxdist, seedlength, palindromic,
                               result);
}

extern "C" int vsa_findselfmatches_edist(const vsa_index *index,
                                         uint64_t leastlength,
                                         uint64_t maxdist,
                                         uint64_t seedlength,
                                         vsa_result **result)
{
  return extend_self<Edist>("vsa_findselfmatches_edist", index, leastlength,
                            maxdist, seedlength, result);
}
