// X-drop extension of exact seeds, vmatch -l L -hxdrop X | -exdrop X
// [-seedlength S] [-p] [-q Q] IDX: every exact seed of a list that stays in
// HBM through xdropseedextend (Vmengine/xdropext.c:39-221).  The rules are
// extend_xdrop_rules.h's, which extend_xdrop_host.c reads too; here is how
// the symbols are read.  Both Multiseqs are flat arrays (extend_flat.hpp).
//
// -hxdrop
//   scan    k_xd_scan: one lane per (seed, side), both texts in words of 8
//           bytes from unaligned starts; the marks of a word -- mismatch,
//           wildcard, separator -- are the events of the rules.  A lane that
//           has looked at `budget` symbols without an end puts its item on
//           the long list.
//   long    k_xd_long: one wavefront per item of the long list, from the
//           start of the side: per step 64 lanes x 16 bytes, a ballot of the
//           lanes that hold a mark, and the marks of those lanes in order
//           through the same events.
// -exdrop
//   gens    k_xd_gens<W>: one group of W = 16, 32 or 64 lanes per (seed,
//           side); lane l is diagonal lower - 1 + l of the current
//           generation.  Per generation: the rows of the three predecessors
//           by shuffles, the entry and the pruning test of the rules (the T
//           values of the last 128 generations in LDS), the slide along both
//           texts in words of 8 bytes, a slide over the budget finished by
//           the group together.  All lanes slide at once under the lengths
//           of the start of the generation; if one of them read a separator,
//           the slides of the generation are done again one after the other
//           in ascending order of the diagonals by the rules' own slide, so
//           that every diagonal sees the lengths (and, to the left, the
//           addressing) the reference's order shows it.  Then the band of the
//           next generation from ballots, and the best score by a reduction
//           in which the lowest diagonal wins among equals.  Only the best
//           (i, j, score) of a side is kept.  A band wider than the group:
//           the item goes to the list of the next width; wider than the
//           widest: the seed is handed over.
// finish    k_xd_finish: one lane per seed, the record and the keep flag by
//           the rules; a seed with a side handed over goes on a list.
// hand-over the seeds of that list (k_xd_gather) are fetched with the two
//           Multiseqs, go through the host rules on several threads
//           (vsa_xd_host_seeds) and k_xd_putback writes their records and
//           keep flags in their places.
// compact   the shared stable compaction: the matches in seed order.
#include "search_host.hpp"
#include "tile_compact.inc"
#include "extend_xdrop_rules.h"
#include "extend_xdrop_host.h"

namespace
{

// the driver, the word load and the words of the counters; EXT_NSTAGE
// counts the sides the long stage scanned (-hxdrop) or with a slide the group
// finished (-exdrop), EXT_SUMLENGTH sums length1 of the matches
#include "extend_shared.hpp"
#include "extend_flat.hpp"

#define XD_BLOCK 256
#define XD_OK 0u
#define XD_MISFIT 1u
#define XD_REJECT 2u
#define XD_HAND 3u

// words of the stage's own counters: items on the two retry lists, seeds
// handed over
#define XD_NLIST0 0
#define XD_NLIST1 1
#define XD_NHAND 2
#define XD_NWORDS 4

struct XdSide
{
  int64_t score;
  uint32_t i, j, status, pad;
};

struct XdParams
{
  const uint8_t *s1, *s2; // the two Multiseqs
  uint64_t n1, n2;
  DevQueries q;
  const uint64_t *abs2; // ragged batches: where the sequences begin in s2
  int self, hamming;
  const vsa_match *seeds;
  uint64_t nseeds, nitems;
  uint64_t leastlength, seedlength;
  uint32_t xdrop, budget;
  XdSide *sides;      // [nitems]
  uint32_t *list[2];  // [nitems] each: the long list / the retry lists
  uint32_t *handlist; // [nseeds]
  uint64_t *handpos2; // [nseeds]
  unsigned long long *counters, *own;
};

// the place of a seed in the second Multiseq; false: it does not fit
__device__ __forceinline__ bool xd_place(const XdParams &p, const vsa_match &m,
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

__device__ __forceinline__ void xd_put(const XdParams &p, uint64_t item,
                                       uint32_t status, const vsa_xd_best &b)
{
  XdSide s;
  s.score = b.score;
  s.i = (uint32_t) b.ivalue;
  s.j = (uint32_t) b.jvalue;
  s.status = status;
  s.pad = 0;
  p.sides[item] = s;
}

// ---- -hxdrop ---------------------------------------------------------------

__device__ __forceinline__ void xd_plan(const XdParams &p, const vsa_match &m,
                                        uint64_t pos2, int left,
                                        vsa_xd_plan &plan)
{
  const vsa_ext_view v1 = {p.s1, p.n1, 1, 1}, v2 = {p.s2, p.n2, 1, 1};
  vsa_xd_prepare(&v1, m.dbstart, &v2, pos2, m.length, left, &plan);
}

__global__ void __launch_bounds__(XD_BLOCK) k_xd_scan(XdParams p)
{
  const uint64_t item = vsa_bid() * XD_BLOCK + threadIdx.x;
  bool tolong = false;

  if (item < p.nitems)
  {
    const vsa_match m = p.seeds[item >> 1];
    const int left = (item & 1) == 0;
    const vsa_xd_best none = {0, 0, 0};
    uint64_t pos2 = 0;

    if (!xd_place(p, m, pos2))
    {
      xd_put(p, item, XD_MISFIT, none);
    } else
    {
      vsa_xd_plan plan;
      vsa_xd_scan s;
      int rc = VSA_XD_ON;
      uint64_t t0 = 0;

      xd_plan(p, m, pos2, left, plan);
      vsa_xd_begin(&s, p.xdrop, p.seedlength, left);
      while (rc == VSA_XD_ON && t0 < plan.nsym && t0 < p.budget)
      {
        uint32_t sep;
        const uint64_t a = ext_word(plan.p1, left, t0, plan.nsym - t0),
                       b = ext_word(plan.p2, left, t0, plan.nsym - t0);
        const uint32_t marks = vsa_ext_marks8(a, b, &sep);
        rc = vsa_xd_events(&s, &plan, t0, marks, sep);
        t0 += 8;
        if (rc == VSA_XD_ON)
        {
          rc = vsa_xd_upto(&s, &plan, t0);
        }
      }
      if (rc == VSA_XD_ON && t0 < plan.nsym)
      {
        tolong = true;
      } else
      {
        vsa_xd_best best;
        if (rc == VSA_XD_ON)
        {
          rc = vsa_xd_finishside(&s, &plan);
        }
        vsa_xd_scanbest(&s, &best);
        xd_put(p, item, rc == VSA_XD_REJECT ? XD_REJECT : XD_OK, best);
      }
    }
  }
  const uint64_t slot = vsa_wave_reserve01(p.counters + EXT_NSTAGE, tolong);
  if (tolong)
  {
    p.list[0][slot] = (uint32_t) item;
  }
}

// sixteen symbols at t0 .. t0 + 15 as two words
__device__ __forceinline__ void xd_word16(const uint8_t *p, int left,
                                          uint64_t t0, uint64_t valid,
                                          uint64_t &w0, uint64_t &w1)
{
  w0 = ext_word(p, left, t0, valid);
  w1 = valid > 8 ? ext_word(p, left, t0 + 8, valid - 8) : 0;
}

__global__ void __launch_bounds__(XD_BLOCK) k_xd_long(XdParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = vsa_nblocks() * (XD_BLOCK / 64),
                 nlong = p.counters[EXT_NSTAGE];

  for (uint64_t w = vsa_bid() * (XD_BLOCK / 64) + (threadIdx.x >> 6);
       w < nlong; w += nwaves)
  {
    const uint32_t item = p.list[0][w];
    const vsa_match m = p.seeds[item >> 1];
    const int left = (item & 1u) == 0;
    vsa_xd_plan plan;
    vsa_xd_scan s;
    vsa_xd_best best;
    uint64_t pos2 = 0;
    int rc = VSA_XD_ON;

    // (the scan stage has seen that the seed fits; every lane keeps the
    // state, lane 0 writes the side)
    if (!xd_place(p, m, pos2))
    {
      continue;
    }
    xd_plan(p, m, pos2, left, plan);
    vsa_xd_begin(&s, p.xdrop, p.seedlength, left);
    for (uint64_t t0 = 0; rc == VSA_XD_ON && t0 < plan.nsym;
         t0 += VSA_EXTEND_LONG_STEP)
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
        xd_word16(plan.p1, left, base, valid, a0, a1);
        xd_word16(plan.p2, left, base, valid, b0, b1);
        marks = vsa_ext_marks8(a0, b0, &s0);
        marks |= vsa_ext_marks8(a1, b1, &s1) << 8;
        seps = s0 | s1 << 8;
        marks &= (1u << valid) - 1u;
      }
      // the lanes that hold a mark, in the order of the symbols
      unsigned long long any = __ballot(marks != 0);
      while (any != 0 && rc == VSA_XD_ON)
      {
        const int l = __ffsll(any) - 1;
        any &= any - 1;
        const uint32_t lm = __shfl(marks, l, 64), ls = __shfl(seps, l, 64);
        rc = vsa_xd_events(&s, &plan, t0 + 16u * (uint32_t) l, lm, ls);
      }
      if (rc == VSA_XD_ON)
      {
        rc = vsa_xd_upto(&s, &plan, t0 + VSA_EXTEND_LONG_STEP);
      }
    }
    if (rc == VSA_XD_ON)
    {
      rc = vsa_xd_finishside(&s, &plan);
    }
    vsa_xd_scanbest(&s, &best);
    if (lane == 0)
    {
      xd_put(p, item, rc == VSA_XD_REJECT ? XD_REJECT : XD_OK, best);
    }
  }
}

// ---- -exdrop ---------------------------------------------------------------

__device__ __forceinline__ int64_t xd_shfl64(int64_t v, int src, int width)
{
  const int lo = __shfl((int) (uint32_t) (uint64_t) v, src, width),
            hi = __shfl((int) (uint32_t) ((uint64_t) v >> 32), src, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

// the marks of the words at offset `at` of a slide from (i0, j0) of which
// `valid` symbols are below the lengths
__device__ __forceinline__ uint32_t xd_marks(const vsa_xd_arrays &a,
                                             int64_t i0, int64_t j0,
                                             int64_t at, int64_t valid)
{
  const uint8_t *pu = a.left ? a.useq + (a.ulen - 1 - i0) : a.useq + i0,
                *pv = a.left ? a.vseq + (a.vlen - 1 - j0) : a.vseq + j0;
  uint32_t sep;
  const uint32_t marks =
      vsa_ext_marks8(ext_word(pu, a.left, (uint64_t) at, (uint64_t) valid),
                     ext_word(pv, a.left, (uint64_t) at, (uint64_t) valid),
                     &sep);
  return valid < 8 ? marks & ((1u << valid) - 1u) : marks;
}

// Every ballot and shuffle below is executed by all lanes of the wavefront:
// the loops run while ANY group of the wavefront has work, and a group
// without work goes through them with nothing to do.
//   list, pn: the items and their number (nullptr: items 0 .. nfixed - 1)
//   retry, nretry: where an item whose band outgrows W lanes goes (nullptr:
//   it is handed over)
template <int W>
__global__ void __launch_bounds__(XD_BLOCK)
k_xd_gens(XdParams p, const uint32_t *__restrict__ list,
          const unsigned long long *__restrict__ pn, uint64_t nfixed,
          uint32_t *__restrict__ retry, unsigned long long *nretry)
{
  static_assert(W == 16 || W == 32 || W == 64, "a group divides a wavefront");
  __shared__ int64_t ringmem[(XD_BLOCK / W) * VSA_XD_RING];
  volatile int64_t *ring = ringmem + (threadIdx.x / W) * VSA_XD_RING;
  const int gl = (int) (threadIdx.x % W);
  // the bits of this group in a ballot
  const uint32_t shift = (threadIdx.x & 63u) & ~(uint32_t) (W - 1);
  const uint64_t groupbits = W == 64 ? ~(uint64_t) 0
                                     : (((uint64_t) 1 << (W & 63)) - 1);
  const uint64_t ngroups = vsa_nblocks() * (XD_BLOCK / W),
                 n = pn != nullptr ? (uint64_t) *pn : nfixed;
  const int64_t xdrop = (int64_t) p.xdrop;

  for (uint64_t w = (vsa_bid() * XD_BLOCK + threadIdx.x) / W;
       __ballot(w < n) != 0; w += ngroups)
  {
    bool active = w < n, first = true, coop = false;
    uint64_t item = 0;
    vsa_xd_arrays a;
    vsa_xd_best best = {0, 0, 0};
    int64_t integermax = 0, minf = 0, lower = 0, upper = 0, prevsmallest = 0,
            dmulti = 0, dback = 0, d = 1, row = 0;

    memset(&a, 0, sizeof a);
    if (active)
    {
      item = list != nullptr ? list[w] : w;
      const vsa_match m = p.seeds[item >> 1];
      uint64_t pos2 = 0;
      if (!xd_place(p, m, pos2))
      {
        active = false;
        if (gl == 0)
        {
          xd_put(p, item, XD_MISFIT, best);
        }
      } else if (!vsa_xd_arrays_init(&a, p.s1, p.n1, p.s2, p.n2, m.dbstart,
                                     pos2, m.length, (item & 1) == 0))
      {
        active = false;
        if (gl == 0)
        {
          xd_put(p, item, XD_OK, best);
        }
      } else
      {
        integermax = a.ulen > a.vlen ? a.ulen : a.vlen;
        minf = -integermax;
        dback = vsa_xd_dback(xdrop);
      }
    }
    while (__ballot(active) != 0)
    {
      // the smallest diagonal of this generation; generation 0 is the
      // slide from (0, 0) on diagonal 0
      const int64_t base = first ? 0 : lower - 1, k = base + gl;
      const int sh = (int) (base - prevsmallest) + gl;
      const int64_t rm1 = xd_shfl64(row, sh - 1, W), r0 = xd_shfl64(row, sh, W),
                    rp1 = xd_shfl64(row, sh + 1, W);
      int64_t i0 = minf, j0 = 0, mlen = 0, rem = 0;
      bool start = false, unfinished = false, read = false;

      if (active && first)
      {
        start = gl == 0;
        i0 = 0;
      } else if (active)
      {
        dmulti += 3;
        if (k <= upper + 1)
        {
          const int64_t dbackvalue =
              dback < 0 ? -xdrop : ring[dback & (VSA_XD_RING - 1)];
          i0 = vsa_xd_entry(k, lower, upper, lower < k ? rm1 : minf,
                            (lower <= k && k <= upper) ? r0 : minf,
                            k < upper ? rp1 : minf, minf);
          if (i0 != minf && vsa_xd_sprime(i0, i0 - k, dmulti) < dbackvalue)
          {
            i0 = minf;
          }
          start = i0 != minf;
        }
      }
      if (start)
      {
        j0 = i0 - k;
        const int64_t ru = a.ulen - i0, rv = a.vlen - j0;
        rem = ru < rv ? ru : rv;
        rem = rem < 0 ? 0 : rem;
        bool done = rem == 0;
        while (!done && mlen < (int64_t) p.budget)
        {
          const int64_t valid = rem - mlen;
          const uint32_t marks = xd_marks(a, i0, j0, mlen, valid);
          if (marks != 0)
          {
            mlen += __builtin_ctz(marks);
            read = true;
            done = true;
          } else
          {
            mlen += valid < 8 ? valid : 8;
            done = mlen >= rem;
          }
        }
        unfinished = !done;
      }
      // the slides that are over the budget, one after the other, by the group
      while (__ballot(unfinished) != 0)
      {
        const uint64_t todo = (__ballot(unfinished) >> shift) & groupbits;
        const int j = todo != 0 ? __ffsll((unsigned long long) todo) - 1 : 0;
        const int64_t ji = xd_shfl64(i0, j, W), jj = xd_shfl64(j0, j, W),
                      jm = xd_shfl64(mlen, j, W), jrem = xd_shfl64(rem, j, W);
        const int64_t at = jm + 8 * (int64_t) gl;
        uint32_t marks = 0;
        if (todo != 0 && at < jrem)
        {
          marks = xd_marks(a, ji, jj, at, jrem - at);
        }
        const uint64_t hit = (__ballot(marks != 0) >> shift) & groupbits;
        const int f = hit != 0 ? __ffsll((unsigned long long) hit) - 1 : 0;
        const uint32_t ffirst =
            (uint32_t) __shfl(marks != 0 ? __builtin_ctz(marks) : 0, f, W);
        if (todo != 0)
        {
          coop = true;
          if (gl == j)
          {
            if (hit != 0)
            {
              mlen = jm + 8 * (int64_t) f + (int64_t) ffirst;
              read = true;
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
      int64_t i = i0 + mlen, j = j0 + mlen;
      bool sep = false;
      if (start && read)
      {
        sep = vsa_xd_usym(&a, i) == (uint8_t) VSA_SEPARATOR ||
              vsa_xd_vsym(&a, j) == (uint8_t) VSA_SEPARATOR;
      }
      bool atN = j == a.vlen, atM = i == a.ulen;
      // a separator was read: the slides in the order of the diagonals,
      // each under the lengths the ones before it left
      if (__ballot(active && sep) != 0)
      {
        const bool mine = ((__ballot(active && sep) >> shift) & groupbits) != 0;
        for (int l = 0; l < W; l++)
        {
          const int lstart = __shfl((int) start, l, W);
          int64_t li = xd_shfl64(i0, l, W), lj = li - (base + l);
          if (mine && lstart)
          {
            vsa_xd_slide(&a, &li, &lj, 0);
            if (gl == l)
            {
              i = li;
              j = lj;
              atN = j == a.vlen;
              atM = i == a.ulen;
            }
          }
        }
      }
      // the best of the generation: the lowest diagonal among equal maxima
      const bool finite = active && start;
      int64_t bs = finite ? vsa_xd_sprime(i, j, dmulti) : INT64_MIN;
      int bl = gl;
#pragma unroll
      for (int x = W / 2; x >= 1; x >>= 1)
      {
        const int64_t os = xd_shfl64(bs, gl ^ x, W);
        const int ol = __shfl(bl, gl ^ x, W);
        if (os > bs || (os == bs && ol < bl))
        {
          bs = os;
          bl = ol;
        }
      }
      const int64_t bi = xd_shfl64(i, bl, W), bj = xd_shfl64(j, bl, W);
      const uint64_t fin = (__ballot(finite) >> shift) & groupbits,
                     nb = (__ballot(finite && atN) >> shift) & groupbits,
                     mb = (__ballot(finite && atM) >> shift) & groupbits;
      if (active)
      {
        row = finite ? i : minf;
        prevsmallest = base;
        if (first)
        {
          first = false;
          best.score = bs;
          best.ivalue = bi;
          best.jvalue = bj;
          if (gl == 0)
          {
            ring[0] = best.score - xdrop;
          }
        } else
        {
          vsa_xd_band band;
          if (fin != 0)
          {
            vsa_xd_better(&best, bi, bj, bs);
          }
          band.minisfinite = fin != 0 ? base + (__ffsll((unsigned long long) fin) - 1)
                                      : integermax;
          band.maxisfinite = fin != 0 ? base + (63 - __clzll((long long) fin))
                                      : -integermax;
          band.maxisN = nb != 0 ? base + (63 - __clzll((long long) nb))
                                : -integermax;
          band.minisM = mb != 0 ? base + (__ffsll((unsigned long long) mb) - 1)
                                : integermax;
          if (vsa_xd_band_next(&band, &lower, &upper))
          {
            active = false;
            if (gl == 0)
            {
              xd_put(p, item, XD_OK, best);
            }
          } else
          {
            if (gl == 0)
            {
              ring[d & (VSA_XD_RING - 1)] = best.score - xdrop;
            }
            d++;
            dback++;
            if (upper - lower + 3 > W)
            {
              // the band outgrows the group
              active = false;
              if (gl == 0)
              {
                if (retry != nullptr)
                {
                  retry[atomicAdd(nretry, 1ull)] = (uint32_t) item;
                } else
                {
                  xd_put(p, item, XD_HAND, best);
                }
              }
            }
          }
        }
      }
      // (the lanes of the group read the ring behind its writer)
      __builtin_amdgcn_wave_barrier();
    }
    if (coop && gl == 0)
    {
      atomicAdd(p.counters + EXT_NSTAGE, 1ull);
    }
  }
}

// ---- both sides together ------------------------------------------------------

__global__ void __launch_bounds__(XD_BLOCK)
k_xd_finish(XdParams p, vsa_match *__restrict__ out, uint8_t *__restrict__ keep)
{
  const uint64_t i = vsa_bid() * XD_BLOCK + threadIdx.x;
  bool misfit = false, hand = false;
  uint64_t len = 0, pos2 = 0;

  if (i < p.nseeds)
  {
    const XdSide ls = p.sides[2 * i], rs = p.sides[2 * i + 1];
    const vsa_match m = p.seeds[i];
    uint8_t kept = 0;
    if (ls.status == XD_MISFIT || rs.status == XD_MISFIT ||
        !xd_place(p, m, pos2))
    {
      misfit = true;
    } else if (ls.status == XD_HAND || rs.status == XD_HAND)
    {
      hand = true;
    } else if (ls.status != XD_REJECT)
    {
      const vsa_xd_best l = {(int64_t) ls.i, (int64_t) ls.j, ls.score},
                        r = {(int64_t) rs.i, (int64_t) rs.j, rs.score};
      vsa_xd_match x;
      if (vsa_xd_finish(p.s1, p.s2, p.self, p.hamming, m.dbstart, pos2,
                        m.length, &l, &r, p.leastlength, &x))
      {
        vsa_match o;
        vsa_xd_record(&m, p.self, pos2, &x, &o);
        out[i] = o;
        len = x.length1;
        kept = 1;
      }
    }
    keep[i] = kept;
  }
  const uint64_t slot = vsa_wave_reserve01(p.own + XD_NHAND, hand);
  if (hand)
  {
    p.handlist[slot] = (uint32_t) i;
    p.handpos2[slot] = pos2;
  }
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

// the seeds of the hand list, side by side
__global__ void __launch_bounds__(XD_BLOCK)
k_xd_gather(uint64_t n, const uint32_t *__restrict__ where,
            const vsa_match *__restrict__ seeds, vsa_match *__restrict__ out)
{
  const uint64_t i = vsa_bid() * XD_BLOCK + threadIdx.x;
  if (i < n)
  {
    out[i] = seeds[where[i]];
  }
}

// the records of the seeds that went through the host rules, in their places
__global__ void __launch_bounds__(XD_BLOCK)
k_xd_putback(uint64_t n, const uint32_t *__restrict__ where,
             const vsa_match *__restrict__ recs,
             const uint8_t *__restrict__ kept, vsa_match *__restrict__ out,
             uint8_t *__restrict__ keep, unsigned long long *counters)
{
  const uint64_t i = vsa_bid() * XD_BLOCK + threadIdx.x;
  if (i < n)
  {
    keep[where[i]] = kept[i];
    if (kept[i])
    {
      out[where[i]] = recs[i];
      atomicAdd(counters + EXT_SUMLENGTH,
                (unsigned long long) VSA_XDROP_LENGTH1(recs[i].length));
    }
  }
}

// host memory of the hand-over (malloc: an entry of the library throws
// nothing)
struct HostBytes
{
  void *p;
  explicit HostBytes(size_t n) : p(malloc(n > 0 ? n : 1)) {}
  ~HostBytes()
  {
    free(p);
  }
  HostBytes(const HostBytes &) = delete;
  HostBytes &operator=(const HostBytes &) = delete;
};

// VSA_EXTEND_XDROP_BAND: the widest group of the device, 16, 32 or 64
int widestband()
{
  const char *e = getenv("VSA_EXTEND_XDROP_BAND");
  const long v = e != nullptr ? strtol(e, nullptr, 10) : 0;
  return (v == 16 || v == 32) ? (int) v : 64;
}

template <int W>
int launchgens(const XdParams &p, const uint32_t *list,
               const unsigned long long *pn, uint64_t most, uint32_t *retry,
               unsigned long long *nretry)
{
  const uint64_t groups = XD_BLOCK / W;
  // (a group per item at most, and no more than fill the device a few times
  // over: the groups take items until the list is done)
  const uint64_t blocks =
      std::min<uint64_t>((most + groups - 1) / groups, 16384);
  k_xd_gens<W><<<vsa_grid(blocks), XD_BLOCK, 0, nullptr>>>(p, list, pn, most,
                                                           retry, nretry);
  VSA_HIP(hipGetLastError());
  return 0;
}

// what the driver of extend_shared.hpp is given; HAMMING: -hxdrop
template <bool HAMMING>
struct Xdrop
{
  static constexpr uint32_t cap = VSA_XDROP_MAXDROP;
  static constexpr bool evalues = false, hequot = false;
  static int checkbound(const char *who, uint64_t xdrop)
  {
    if (xdrop > VSA_XDROP_MAXDROP)
    {
      VSA_ERROR("%s: X = %lu: the reference takes 1 to %u (FLAGXDROP, "
                "Vmatch/parsevm.c)", who, (unsigned long) xdrop,
                VSA_XDROP_MAXDROP);
      return -2;
    }
    return 0;
  }
  static uint64_t seedlength(uint64_t, uint64_t, uint64_t seedlength)
  {
    return vsa_xd_seedlength(seedlength);
  }

  struct Stage
  {
    Timer tfirst{nullptr}, tsecond{nullptr};
    XdParams p;
    DevBuf flat, abs2, sides, list0, list1, handlist, handpos2, own;
    uint64_t handed = 0;

    int prepare(const ExtCall &c, Timer &tall)
    {
      memset(&p, 0, sizeof p);
      p.s1 = c.index->tis_alloc + VSA_TIS_FRONTPAD;
      p.n1 = c.index->n;
      p.self = c.self;
      p.hamming = HAMMING;
      p.seeds = c.seeds->matches;
      p.nseeds = c.seeds->count;
      p.nitems = 2 * c.seeds->count;
      p.leastlength = c.leastlength;
      p.seedlength = c.seedlength;
      p.xdrop = (uint32_t) c.maxdist;
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
      if (sides.alloc(p.nitems * sizeof(XdSide)) != 0 ||
          list0.alloc(p.nitems * 4) != 0 ||
          (!HAMMING && list1.alloc(p.nitems * 4) != 0) ||
          handlist.alloc(p.nseeds * 4) != 0 ||
          handpos2.alloc(p.nseeds * 8) != 0 || own.alloc(XD_NWORDS * 8) != 0)
      {
        return -100;
      }
      p.sides = sides.as<XdSide>();
      p.list[0] = list0.as<uint32_t>();
      p.list[1] = list1.as<uint32_t>();
      p.handlist = handlist.as<uint32_t>();
      p.handpos2 = handpos2.as<uint64_t>();
      p.own = own.as<unsigned long long>();
      return 0;
    }

    // The seeds of the hand list through the host rules.  Only they are
    // fetched, gathered on the device; the two Multiseqs come whole, because
    // the arrays of a side are "everything in front of / behind the seed".
    int handover(const ExtCall &c, vsa_match *recs, uint8_t *keep)
    {
      const uint64_t n = handed;
      DevBuf dseeds, dout, dkept;
      if (dseeds.alloc(n * sizeof(vsa_match)) != 0 ||
          dout.alloc(n * sizeof(vsa_match)) != 0 || dkept.alloc(n) != 0)
      {
        return -100;
      }
      k_xd_gather<<<vsa_grid((n + XD_BLOCK - 1) / XD_BLOCK), XD_BLOCK, 0,
                    nullptr>>>(n, p.handlist, p.seeds, dseeds.as<vsa_match>());
      VSA_HIP(hipGetLastError());
      HostBytes pos2(n * 8), seeds(n * sizeof(vsa_match)),
          out(n * sizeof(vsa_match)), kept(n), s1(p.n1),
          s2(c.self ? 0 : p.n2);
      if (!pos2.p || !seeds.p || !out.p || !kept.p || !s1.p || !s2.p)
      {
        VSA_ERROR("out of memory");
        return -101;
      }
      VSA_HIP(hipMemcpy(pos2.p, p.handpos2, n * 8, hipMemcpyDeviceToHost));
      VSA_HIP(hipMemcpy(seeds.p, dseeds.p, n * sizeof(vsa_match),
                        hipMemcpyDeviceToHost));
      VSA_HIP(hipMemcpy(s1.p, p.s1, p.n1, hipMemcpyDeviceToHost));
      if (!c.self && p.n2 > 0)
      {
        VSA_HIP(hipMemcpy(s2.p, p.s2, p.n2, hipMemcpyDeviceToHost));
      }
      const int rc = vsa_xd_host_seeds(
          (const uint8_t *) s1.p, p.n1,
          (const uint8_t *) (c.self ? s1.p : s2.p), p.n2, c.self, HAMMING,
          (const vsa_match *) seeds.p, (const uint64_t *) pos2.p, n,
          c.leastlength, c.maxdist, c.seedlength, 0, (vsa_match *) out.p,
          (uint8_t *) kept.p);
      if (rc != 0)
      {
        return rc;
      }
      VSA_HIP(hipMemcpy(dout.p, out.p, n * sizeof(vsa_match),
                        hipMemcpyHostToDevice));
      VSA_HIP(hipMemcpy(dkept.p, kept.p, n, hipMemcpyHostToDevice));
      k_xd_putback<<<vsa_grid((n + XD_BLOCK - 1) / XD_BLOCK), XD_BLOCK, 0,
                     nullptr>>>(n, p.handlist, dout.as<vsa_match>(),
                                dkept.as<uint8_t>(), recs, keep, p.counters);
      VSA_HIP(hipGetLastError());
      VSA_HIP(hipStreamSynchronize(nullptr));
      return 0;
    }

    int run(const ExtCall &c, vsa_match *recs, uint8_t *keep,
            unsigned long long *counters, Timer &, Timer &tsearch)
    {
      p.counters = counters;
      VSA_HIP(hipMemsetAsync(counters, 0, EXT_NCOUNTERS * 8, nullptr));
      VSA_HIP(hipMemsetAsync(p.own, 0, XD_NWORDS * 8, nullptr));
      tsearch.start();
      tfirst.start();
      if (HAMMING)
      {
        k_xd_scan<<<vsa_grid((p.nitems + XD_BLOCK - 1) / XD_BLOCK), XD_BLOCK,
                    0, nullptr>>>(p);
        VSA_HIP(hipGetLastError());
        tfirst.stop();
        const uint64_t longblocks = std::min<uint64_t>(
            (p.nitems + XD_BLOCK / 64 - 1) / (XD_BLOCK / 64), 8192);
        tsecond.start();
        k_xd_long<<<vsa_grid(longblocks), XD_BLOCK, 0, nullptr>>>(p);
        VSA_HIP(hipGetLastError());
        tsecond.stop();
      } else
      {
        // every side by a group of 16; what outgrows it by 32, then by 64
        const int widest = widestband();
        int rc = launchgens<16>(p, nullptr, nullptr, p.nitems,
                                widest > 16 ? p.list[0] : nullptr,
                                p.own + XD_NLIST0);
        tfirst.stop();
        tsecond.start();
        if (rc == 0 && widest > 16)
        {
          rc = launchgens<32>(p, p.list[0], p.own + XD_NLIST0, p.nitems,
                              widest > 32 ? p.list[1] : nullptr,
                              p.own + XD_NLIST1);
        }
        if (rc == 0 && widest > 32)
        {
          rc = launchgens<64>(p, p.list[1], p.own + XD_NLIST1, p.nitems,
                              nullptr, nullptr);
        }
        tsecond.stop();
        if (rc != 0)
        {
          return rc;
        }
      }
      k_xd_finish<<<vsa_grid((p.nseeds + XD_BLOCK - 1) / XD_BLOCK), XD_BLOCK,
                    0, nullptr>>>(p, recs, keep);
      VSA_HIP(hipGetLastError());
      tsearch.stop();
      unsigned long long words[XD_NWORDS];
      VSA_HIP(hipMemcpy(words, p.own, sizeof words, hipMemcpyDeviceToHost));
      handed = words[XD_NHAND];
      return handed > 0 ? handover(c, recs, keep) : 0;
    }

    void stats(vsa_stats &st)
    {
      st.first_kernel_ms = tfirst.ms();
      st.anchor_ms = tsecond.ms();
      st.kernel_searches = handed;
    }
  };
};

} // namespace

extern "C" uint64_t vsa_extend_xdrop_seedlength(uint64_t seedlength)
{
  return vsa_xd_seedlength(seedlength);
}

extern "C" int vsa_extend_xdrop(const vsa_index *index,
                                const vsa_queries *queries,
                                const vsa_result *seeds,
                                const vsa_sinkparams *layout, int palindromic,
                                uint64_t leastlength, uint64_t xdrop,
                                int hamming, uint64_t seedlength,
                                vsa_result **result)
{
  const char *who = "vsa_extend_xdrop";
  return hamming ? extend_list<Xdrop<true>>(who, index, queries, seeds, layout,
                                            palindromic, leastlength, xdrop,
                                            seedlength, result)
                 : extend_list<Xdrop<false>>(who, index, queries, seeds,
                                             layout, palindromic, leastlength,
                                             xdrop, seedlength, result);
}

extern "C" int vsa_findquerymatches_xdrop(const vsa_index *index,
                                          const vsa_queries *queries,
                                          uint64_t leastlength, uint64_t xdrop,
                                          int hamming, uint64_t seedlength,
                                          int palindromic,
                                          vsa_result **result)
{
  const char *who = "vsa_findquerymatches_xdrop";
  return hamming ? extend_queries<Xdrop<true>>(who, index, queries,
                                               leastlength, xdrop, seedlength,
                                               palindromic, result)
                 : extend_queries<Xdrop<false>>(who, index, queries,
                                                leastlength, xdrop,
                                                seedlength, palindromic,
                                                result);
}

extern "C" int vsa_findselfmatches_xdrop(const vsa_index *index,
                                         uint64_t leastlength, uint64_t xdrop,
                                         int hamming, uint64_t seedlength,
                                         vsa_result **result)
{
  const char *who = "vsa_findselfmatches_xdrop";
  return hamming ? extend_self<Xdrop<true>>(who, index, leastlength, xdrop,
                                            seedlength, result)
                 : extend_self<Xdrop<false>>(who, index, leastlength, xdrop,
                                             seedlength, result);
}
