// Alignments of degenerate matches, vmatch -s: the edit script of every record
// of a match list that stays in HBM.  The rules are align_rules.h's, which
// align_host.c reads too; here is how the scripts are made.
//
//   flatten k_flatten (extend_flat.hpp): the query batch as the reference's
//           Multiseq.  For a palindromic list nothing is reversed: the right
//           substring is read backwards in the forward sequence and
//           complemented a word at a time (al_complement8).
//   count   k_al_count: one lane per record.  The view of the record, whether
//           it fits its texts, the largest stored distance of the list, and
//           the room of its script: the bound of the rules for a record of
//           positive distance, the exact number of words for one of distance
//           0; a -h record gets its number from k_al_hamming<false>.
//   fronts  k_al_fronts<W>: one group of W = 16, 32 or 64 lanes per record of
//           positive distance, chosen by 2 D + 1 for the largest stored
//           distance D of the list; lane l is the diagonal l - D.  The rows of
//           the neighbouring diagonals come by shuffles, the slides run in
//           words of 8 bytes; a slide that has not ended after `budget`
//           symbols is finished by the group together (as in k_ed_fronts).
//           EVERY LANE KEEPS THE DIRECTIONS OF ITS DIAGONAL IN ONE 64-BIT
//           REGISTER, two bits per generation: no front goes to memory, and
//           the list is not cut into pieces.  The end test is one shuffle of
//           the row of lane vlen - ulen + D per generation.  The backtrace
//           follows in the same kernel: the direction word of the current
//           diagonal comes by a shuffle, the backward slide is done by the
//           group -- every lane one word, a ballot finds the first
//           difference --, lane 0 writes the words.
//   hamming k_al_hamming<WRITE>: one wavefront per record of distance <= 0:
//           the marks of 64 words, a ballot, the runs between the marks.
//   deliver exclusive sums of the rooms and of the words written
//           (exclusive_sum, search_common.hip); k_al_gather copies the
//           scripts into a tight array in the order of the records.  A list
//           without a record of positive distance is tight as it is written.
// Nothing is read through a record that does not fit its texts: such a record
// is counted by k_al_count and the call fails before another kernel runs.
#include "resident_list.hpp"
#include "tile_compact.inc"
#include "extend_rules.h"
#include "align_rules.h"

namespace
{

// ext_word, lanebudget (VSA_EXTEND_STAGE)
#include "extend_shared.hpp"
// the query Multiseq (k_flatten)
#include "extend_flat.hpp"

#define AL_BLOCK 256

static_assert(VSA_ALIGN_MAXDIST + 1 <= VSA_AL_REGISTERGENS &&
                  2 * VSA_AL_REGISTERGENS == 64,
              "two bits per generation: the directions of a diagonal over the "
              "generations 0 .. VSA_ALIGN_MAXDIST are one 64-bit register");
static_assert(2 * VSA_ALIGN_MAXDIST + 1 <= 64,
              "the diagonals of a front are the lanes of one wavefront");

// words of the counters
#define AL_NMISFIT 0   // records that do not fit their texts
#define AL_MAXDIST 1   // the largest stored distance > 0
#define AL_NEDIST 2    // records of positive distance
#define AL_NOTHER 3    // ... of distance <= 0
#define AL_NABOVE 4    // records whose edit distance is above the stored one
#define AL_NSTAGE 5    // groups that finished a slide together
#define AL_NOROOM 6    // scripts that left their room (none, by the bound)
#define AL_NCOUNTERS 7

struct AlParams
{
  const uint8_t *s1, *s2; // the index and the query Multiseq
  uint64_t n1, n2;
  DevQueries q;
  const uint64_t *abs2; // ragged batches: where the sequences begin in s2
  int kind, self, palindromic;
  const vsa_match *recs;
  uint64_t count;
  uint32_t maxdist, budget;
  uint64_t *room;         // [count + 1]: words a script may take
  const uint64_t *tmpoff; // [count + 1]: their exclusive sums
  uint16_t *tmp;          // the scripts, each in its room
  uint64_t *cnt;          // [count + 1]: words of each script
  unsigned long long *counters;
};

// the view and the two substrings of a record; false: it does not fit
__device__ __forceinline__ bool al_place(const AlParams &p, const vsa_match &m,
                                         vsa_al_view &w, vsa_al_pair &pr)
{
  uint64_t seqlength2 = 0, qabs = 0;

  if (!p.self)
  {
    if (m.queryseq < p.q.seqoffset || m.queryseq - p.q.seqoffset >= p.q.nq)
    {
      return false;
    }
    const uint64_t qi = m.queryseq - p.q.seqoffset;
    seqlength2 = flat_qlength(p, qi);
    qabs = flat_qabs(p, qi);
  }
  if (vsa_al_viewof(p.kind, &m, seqlength2, &w) != 0 ||
      !vsa_al_fits(&w, m.dbstart, p.n1, p.self ? p.n1 : seqlength2))
  {
    return false;
  }
  pr.u = p.s1 + m.dbstart;
  pr.ulen = w.length1;
  pr.vlen = w.length2;
  pr.vrev = 0;
  pr.onearray = 0;
  pr.pu = pr.pv = 0;
  if (p.self)
  {
    pr.v = p.s1 + w.start2;
    pr.onearray = 1;
    pr.pu = m.dbstart;
    pr.pv = w.start2;
  } else
  {
    pr.v = p.s2 + qabs + vsa_al_vfirst(&w, seqlength2, p.palindromic);
    pr.vrev = p.palindromic;
  }
  return true;
}

// vsa_al_complement of the eight bytes of a word
__device__ __forceinline__ uint64_t al_complement8(uint64_t c)
{
  const uint64_t special = (c >> 7 & 0x0101010101010101ull) * 3u;
  return c ^ (0x0303030303030303ull & ~special);
}

// the marks of the words at offset `at` of the FORWARD slide from (t, t + k),
// of which `valid` symbols are below the bounds
__device__ __forceinline__ uint32_t al_marks(const vsa_al_pair &pr, int64_t t,
                                             int64_t k, int64_t at,
                                             int64_t valid)
{
  uint32_t sep;
  const uint64_t a = ext_word(pr.u + t, 0, (uint64_t) at, (uint64_t) valid);
  uint64_t c = ext_word(pr.vrev ? pr.v - (t + k) : pr.v + (t + k), pr.vrev,
                        (uint64_t) at, (uint64_t) valid);
  if (pr.vrev)
  {
    c = al_complement8(c);
  }
  const uint32_t marks = vsa_ext_marks8(a, c, &sep);
  return valid < 8 ? marks & ((1u << valid) - 1u) : marks;
}

// ... of the BACKWARD slide from (i, j): symbol x of the word is (i - at - x,
// j - at - x)
__device__ __forceinline__ uint32_t al_marksback(const vsa_al_pair &pr,
                                                 int64_t i, int64_t j,
                                                 int64_t at, int64_t valid)
{
  uint32_t sep;
  const uint64_t a = ext_word(pr.u + i, 1, (uint64_t) at, (uint64_t) valid);
  uint64_t c = ext_word(pr.vrev ? pr.v - j : pr.v + j, !pr.vrev,
                        (uint64_t) at, (uint64_t) valid);
  if (pr.vrev)
  {
    c = al_complement8(c);
  }
  const uint32_t marks = vsa_ext_marks8(a, c, &sep);
  return valid < 8 ? marks & ((1u << valid) - 1u) : marks;
}

__device__ __forceinline__ int64_t al_shfl64(int64_t v, int src, int width)
{
  const int lo = __shfl((int) (uint32_t) (uint64_t) v, src, width),
            hi = __shfl((int) (uint32_t) ((uint64_t) v >> 32), src, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

// a script under construction: lane 0 of a group or wavefront writes, every
// lane counts.  A word that would leave the room is counted, not written.
struct AlScript
{
  uint16_t *out;
  uint64_t room, n;
  bool writes;

  __device__ __forceinline__ void put(uint16_t w)
  {
    if (writes && n < room)
    {
      out[n] = w;
    }
    n++;
  }
  __device__ __forceinline__ void identical(uint64_t lenid)
  {
    const uint64_t pieces = vsa_al_identical(nullptr, lenid);
    if (writes && n + pieces <= room)
    {
      (void) vsa_al_identical(out + n, lenid);
    }
    n += pieces;
  }
};

__global__ void __launch_bounds__(AL_BLOCK) k_al_count(AlParams p)
{
  const uint64_t i = vsa_bid() * AL_BLOCK + threadIdx.x;
  bool misfit = false, edist = false, other = false;
  unsigned long long dist = 0;

  if (i < p.count)
  {
    vsa_al_view w;
    vsa_al_pair pr;
    uint64_t room = 0;
    if (!al_place(p, p.recs[i], w, pr))
    {
      misfit = true;
    } else if (w.distance > 0)
    {
      edist = true;
      dist = (unsigned long long) w.distance;
      room = vsa_al_maxwords((uint64_t) w.distance, pr.ulen, pr.vlen);
    } else
    {
      other = true;
      room = w.distance == 0 ? vsa_al_identical(nullptr, pr.ulen) : 0;
    }
    p.room[i] = room;
    p.cnt[i] = 0;
  }
  // (every lane of the wavefront is here)
  wave_count(misfit, p.counters + AL_NMISFIT);
  wave_count(edist, p.counters + AL_NEDIST);
  wave_count(other, p.counters + AL_NOTHER);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    const unsigned long long o =
        vsa_shfl64(dist, (int) ((threadIdx.x & 63u) ^ (uint32_t) d));
    dist = o > dist ? o : dist;
  }
  if ((threadIdx.x & 63u) == 0 && dist != 0)
  {
    atomicMax(p.counters + AL_MAXDIST, dist);
  }
}

// Every ballot and shuffle below is executed by all lanes of the wavefront:
// the loops run while ANY group of the wavefront has work, and a group
// without work goes through them with nothing to do.
template <int W>
__global__ void __launch_bounds__(AL_BLOCK) k_al_fronts(AlParams p)
{
  static_assert(W == 16 || W == 32 || W == 64, "a group divides a wavefront");
  const uint64_t g = (vsa_bid() * AL_BLOCK + threadIdx.x) / W;
  const int gl = (int) (threadIdx.x % W);
  // the bits of this group in a ballot
  const uint32_t shift = (threadIdx.x & 63u) & ~(uint32_t) (W - 1);
  const uint64_t groupbits = W == 64 ? ~(uint64_t) 0
                                     : (((uint64_t) 1 << (W & 63)) - 1);
  const int64_t D = (int64_t) p.maxdist;
  const int64_t k = (int64_t) gl - D;
  bool active = false, coop = false;
  vsa_al_view w;
  vsa_al_pair pr;
  AlScript s;
  int64_t row = VSA_ER_NEG, stored = 0, enddiag = 0, real = -1;
  uint64_t dirs = 0;

  memset(&pr, 0, sizeof pr);
  memset(&w, 0, sizeof w);
  s.out = nullptr;
  s.room = s.n = 0;
  s.writes = false;
  if (g < p.count && al_place(p, p.recs[g], w, pr) && w.distance > 0 &&
      w.distance <= D)
  {
    active = true;
    stored = w.distance;
    enddiag = (int64_t) pr.vlen - (int64_t) pr.ulen;
    s.out = p.tmp + p.tmpoff[g];
    s.room = p.tmpoff[g + 1] - p.tmpoff[g];
    s.writes = gl == 0;
  }
  // ---- the fronts: generation 0 is the slide of diagonal 0 from row 0 ----
  for (int64_t gen = 0; __ballot(active) != 0; gen++)
  {
    // (the outermost lanes take minus infinity instead, below)
    const int64_t below = al_shfl64(row, (gl + W - 1) % W, W),
                  above = al_shfl64(row, (gl + 1) % W, W);
    int64_t t = 0, mlen = 0, rem = 0, value = row;
    bool slides = false, unfinished = false;

    if (active && k >= -gen && k <= gen)
    {
      if (gen == 0)
      {
        slides = true;
      } else
      {
        const int dir = vsa_al_direction(row, gl == 0 ? VSA_ER_NEG : below,
                                         gl == W - 1 ? VSA_ER_NEG : above, &t);
        dirs = vsa_al_setdir(dirs, gen, dir);
        slides = !vsa_al_noslide(&pr, t, k, &value);
      }
      if (slides)
      {
        const int64_t ru = (int64_t) pr.ulen - t,
                      rv = (int64_t) pr.vlen - (t + k);
        rem = ru < rv ? ru : rv;
        rem = rem < 0 ? 0 : rem;
        bool done = rem == 0;
        while (!done && mlen < (int64_t) p.budget)
        {
          const int64_t valid = rem - mlen;
          const uint32_t marks = al_marks(pr, t, k, mlen, valid);
          if (marks != 0)
          {
            mlen += (int64_t) __builtin_ctz(marks);
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
      const int64_t jt = al_shfl64(t, j, W), jm = al_shfl64(mlen, j, W),
                    jrem = al_shfl64(rem, j, W), jk = (int64_t) j - D;
      const int64_t at = jm + 8 * (int64_t) gl;
      uint32_t marks = 0;
      if (todo != 0 && at < jrem)
      {
        marks = al_marks(pr, jt, jk, at, jrem - at);
      }
      const uint64_t hit = (__ballot(marks != 0) >> shift) & groupbits;
      const int f = hit != 0 ? __ffsll((unsigned long long) hit) - 1 : 0;
      const uint32_t ffirst = (uint32_t) __shfl(
          marks != 0 ? (int) __builtin_ctz(marks) : 0, f, W);
      if (todo != 0)
      {
        coop = true;
        if (gl == j)
        {
          if (hit != 0)
          {
            mlen = jm + 8 * (int64_t) f + (int64_t) ffirst;
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
    if (slides)
    {
      value = vsa_er_stored(t + mlen, k, pr.ulen, pr.vlen);
    }
    row = value;
    const int64_t endrow = al_shfl64(row, (int) (enddiag + D), W);
    if (active)
    {
      if (vsa_al_ends(endrow, pr.ulen))
      {
        real = gen;
        active = false;
      } else if (gen == stored)
      {
        active = false; // the edit distance is above the stored one
      }
    }
  }
  // ---- the backtrace ----------------------------------------------------------
  bool tracing = real >= 0;
  int64_t gen = real, i = (int64_t) pr.ulen - 1, j = (int64_t) pr.vlen - 1,
          d = enddiag;
  while (__ballot(tracing) != 0)
  {
    // the backward slide of the group: every lane one word per round
    int64_t run = 0;
    bool sliding = tracing && gen > 0;
    const int64_t brem = sliding && i >= 0 && j >= 0 ? (i < j ? i : j) + 1 : 0;
    while (__ballot(sliding) != 0)
    {
      const int64_t at = run + 8 * (int64_t) gl;
      uint32_t marks = 0;
      if (sliding && at < brem)
      {
        marks = al_marksback(pr, i, j, at, brem - at);
      }
      const uint64_t hit = (__ballot(marks != 0) >> shift) & groupbits;
      const int f = hit != 0 ? __ffsll((unsigned long long) hit) - 1 : 0;
      const uint32_t ffirst = (uint32_t) __shfl(
          marks != 0 ? (int) __builtin_ctz(marks) : 0, f, W);
      if (sliding)
      {
        if (hit != 0)
        {
          run += 8 * (int64_t) f + (int64_t) ffirst;
          sliding = false;
        } else if (run + 8 * W >= brem)
        {
          run = brem;
          sliding = false;
        } else
        {
          run += 8 * W;
        }
      }
    }
    // the direction of front(gen, d), kept by lane d + D
    const int64_t dirword = al_shfl64((int64_t) dirs, (int) (d + D), W);
    if (tracing)
    {
      if (gen > 0)
      {
        i -= run;
        j -= run;
        if (run > 0)
        {
          s.identical((uint64_t) run);
        }
        s.put(vsa_al_step(vsa_al_getdir((uint64_t) dirword, gen), &i, &j, &d));
        gen--;
      }
      if (gen == 0)
      {
        if (i >= 0)
        {
          s.identical((uint64_t) i + 1);
        }
        tracing = false;
      }
    }
  }
  if (gl == 0 && g < p.count && stored > 0)
  {
    const bool noroom = s.n > s.room;
    p.cnt[g] = real >= 0 && !noroom ? s.n : 0;
    if (real < 0)
    {
      atomicAdd(p.counters + AL_NABOVE, 1ull);
    }
    if (noroom)
    {
      atomicAdd(p.counters + AL_NOROOM, 1ull);
    }
    if (coop)
    {
      atomicAdd(p.counters + AL_NSTAGE, 1ull);
    }
  }
}

// one wavefront per record of distance <= 0; !WRITE: the room of a -h record
template <bool WRITE>
__global__ void __launch_bounds__(AL_BLOCK) k_al_hamming(AlParams p)
{
  const uint64_t r = (vsa_bid() * AL_BLOCK + threadIdx.x) / 64;
  const int lane = (int) (threadIdx.x & 63u);
  vsa_al_view w;
  vsa_al_pair pr;

  // (r, and with it every branch below but the marks, is one for the
  // wavefront)
  if (r >= p.count || !al_place(p, p.recs[r], w, pr) || w.distance > 0 ||
      (!WRITE && w.distance == 0))
  {
    return;
  }
  AlScript s;
  s.out = WRITE ? p.tmp + p.tmpoff[r] : nullptr;
  s.room = WRITE ? p.tmpoff[r + 1] - p.tmpoff[r] : 0;
  s.n = 0;
  s.writes = WRITE && lane == 0;
  if (w.distance == 0)
  {
    s.identical(pr.ulen);
  } else
  {
    const int64_t len = (int64_t) pr.ulen;
    uint64_t carry = 0; // the identical run so far
    for (int64_t base = 0; base < len; base += 512)
    {
      const int64_t at = base + 8 * (int64_t) lane;
      const uint32_t marks =
          at < len ? al_marksback(pr, len - 1, len - 1, at, len - at) : 0;
      uint64_t hits = __ballot(marks != 0);
      int64_t pos = base; // symbols from the back accounted for
      while (hits != 0)
      {
        const int l = __ffsll((unsigned long long) hits) - 1;
        uint32_t mk = (uint32_t) __shfl((int) marks, l);
        hits &= hits - 1;
        while (mk != 0)
        {
          const int64_t at1 = base + 8 * (int64_t) l + __builtin_ctz(mk);
          mk &= mk - 1;
          carry += (uint64_t) (at1 - pos);
          if (carry > 0)
          {
            s.identical(carry);
            carry = 0;
          }
          s.put(VSA_AL_MISMATCH);
          pos = at1 + 1;
        }
      }
      carry += (uint64_t) ((base + 512 < len ? base + 512 : len) - pos);
    }
    if (carry > 0)
    {
      s.identical(carry);
    }
  }
  if (lane == 0)
  {
    if (WRITE)
    {
      p.cnt[r] = s.n <= s.room ? s.n : 0;
      if (s.n > s.room)
      {
        atomicAdd(p.counters + AL_NOROOM, 1ull);
      }
    } else
    {
      p.room[r] = s.n;
    }
  }
}

__global__ void __launch_bounds__(AL_BLOCK)
k_al_gather(const uint16_t *__restrict__ tmp,
            const uint64_t *__restrict__ tmpoff,
            const uint64_t *__restrict__ offsets, uint64_t count,
            uint16_t *__restrict__ eops)
{
  const uint64_t i = vsa_bid() * AL_BLOCK + threadIdx.x;
  if (i < count)
  {
    const uint64_t n = offsets[i + 1] - offsets[i];
    const uint16_t *src = tmp + tmpoff[i];
    uint16_t *dst = eops + offsets[i];
    for (uint64_t x = 0; x < n; x++)
    {
      dst[x] = src[x];
    }
  }
}

template <int W>
int launchfronts(const AlParams &p)
{
  const uint64_t groups = AL_BLOCK / W;
  k_al_fronts<W><<<vsa_grid((p.count + groups - 1) / groups), AL_BLOCK, 0,
                   nullptr>>>(p);
  VSA_HIP(hipGetLastError());
  return 0;
}

} // namespace

struct vsa_alignments
{
  int device;
  uint64_t *offsets; // device [count + 1]
  uint16_t *eops;    // device [words]
  vsa_alignstats stats;
};

extern "C" uint32_t vsa_align_maxdist(void)
{
  return VSA_ALIGN_MAXDIST;
}

extern "C" int vsa_align(const vsa_index *index, const vsa_queries *queries,
                         const vsa_result *matches,
                         const vsa_sinkparams *layout, int palindromic,
                         vsa_alignments **alignments)
{
  static const char who[] = "vsa_align";

  if (index == nullptr || matches == nullptr || layout == nullptr ||
      alignments == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  *alignments = nullptr;
  if (layout->selfpalindromic)
  {
    VSA_ERROR("%s: lists of vmatch -p IDX (selfpalindromic) are not covered",
              who);
    return VSA_NOT_COVERED;
  }
  if (!vsa_al_covered(layout->kind))
  {
    VSA_ERROR("%s: a layout of kind %d (X-drop extended seeds, a six-frame "
              "translated batch) is not covered", who, layout->kind);
    return VSA_NOT_COVERED;
  }
  if (matches->packbits != 0)
  {
    VSA_ERROR("%s: a packed candidate result has no records to align", who);
    return VSA_NOT_COVERED;
  }
  const bool self = vsa_al_isself(layout->kind);
  if (self != (queries == nullptr) || (self && palindromic) ||
      (palindromic && index->numofchars != 4))
  {
    VSA_ERROR("%s: a query layout with its batch (palindromic: over 4 "
              "characters) or a self layout without one, not palindromic",
              who);
    return -2;
  }
  if (index->n >= 0xFFFFFFF0ull ||
      (queries != nullptr && queries->maxlength >= 0xFFFFFFF0ull))
  {
    VSA_ERROR("%s: texts and query sequences below 2^32 - 16 symbols are "
              "covered", who);
    return VSA_NOT_COVERED;
  }
  if (matches->count >= (1ull << 31))
  {
    VSA_ERROR("%s: %lu records: fewer than 2^31 are covered", who,
              (unsigned long) matches->count);
    return VSA_NOT_COVERED;
  }
  if (matches->device != index->device ||
      (queries != nullptr && queries->device != index->device))
  {
    VSA_ERROR("%s: index, batch and list on one device", who);
    return -2;
  }
  if (enter(index->device) != 0)
  {
    return -100;
  }
  const uint64_t n = matches->count;
  DevBuf flat, abs2, counters, room, tmpoff, tmp, cnt, offsets, eops;
  AlParams p;
  Timer tall(nullptr), tkernel(nullptr);
  memset(&p, 0, sizeof p);
  p.s1 = index->tis_alloc + VSA_TIS_FRONTPAD;
  p.n1 = index->n;
  p.kind = layout->kind;
  p.self = self;
  p.palindromic = palindromic != 0;
  p.recs = matches->matches;
  p.count = n;
  p.budget = lanebudget();
  if (offsets.alloc((n + 1) * 8) != 0)
  {
    return -100;
  }
  uint64_t words = 0, cw[AL_NCOUNTERS];
  memset(cw, 0, sizeof cw);
  tall.start();
  if (n == 0)
  {
    VSA_HIP(hipMemsetAsync(offsets.p, 0, 8, nullptr));
  } else
  {
    if (!self)
    {
      if (vsa_queries_bytes(queries, nullptr) != 0)
      {
        return -100;
      }
      const int rc = flatten_batch(who, queries, p, flat, abs2);
      if (rc != 0)
      {
        return rc;
      }
    }
    if (counters.alloc(AL_NCOUNTERS * 8) != 0 ||
        room.alloc((n + 1) * 8) != 0 || tmpoff.alloc((n + 1) * 8) != 0 ||
        cnt.alloc((n + 1) * 8) != 0)
    {
      return -100;
    }
    p.counters = counters.as<unsigned long long>();
    p.room = room.as<uint64_t>();
    p.cnt = cnt.as<uint64_t>();
    VSA_HIP(hipMemsetAsync(counters.p, 0, AL_NCOUNTERS * 8, nullptr));
    VSA_HIP(hipMemsetAsync(p.room + n, 0, 8, nullptr));
    VSA_HIP(hipMemsetAsync(p.cnt + n, 0, 8, nullptr));
    k_al_count<<<vsa_grid((n + AL_BLOCK - 1) / AL_BLOCK), AL_BLOCK, 0,
                 nullptr>>>(p);
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(cw, counters.p, sizeof cw, hipMemcpyDeviceToHost));
    if (cw[AL_NMISFIT] != 0)
    {
      VSA_ERROR("%s: %lu records do not fit the index or their query "
                "sequence, or name a match no matcher delivers", who,
                (unsigned long) cw[AL_NMISFIT]);
      return -2;
    }
    if (cw[AL_MAXDIST] > VSA_ALIGN_MAXDIST)
    {
      VSA_ERROR("%s: a stored distance of %lu: up to %u are covered on the "
                "device (vsa_align_host takes any)", who,
                (unsigned long) cw[AL_MAXDIST], VSA_ALIGN_MAXDIST);
      return VSA_NOT_COVERED;
    }
    p.maxdist = (uint32_t) cw[AL_MAXDIST];
    const uint64_t waves = (n + AL_BLOCK / 64 - 1) / (AL_BLOCK / 64);
    if (cw[AL_NOTHER] != 0)
    {
      k_al_hamming<false><<<vsa_grid(waves), AL_BLOCK, 0, nullptr>>>(p);
      VSA_HIP(hipGetLastError());
    }
    uint64_t tmpwords = 0;
    if (exclusive_sum(p.room, tmpoff.as<uint64_t>(), n, nullptr,
                      &tmpwords) != 0 ||
        tmp.alloc(tmpwords * 2) != 0)
    {
      return -100;
    }
    p.tmpoff = tmpoff.as<uint64_t>();
    p.tmp = tmp.as<uint16_t>();
    tkernel.start();
    if (cw[AL_NEDIST] != 0)
    {
      const int rc = p.maxdist <= 7    ? launchfronts<16>(p)
                     : p.maxdist <= 15 ? launchfronts<32>(p)
                                       : launchfronts<64>(p);
      if (rc != 0)
      {
        return rc;
      }
    }
    if (cw[AL_NOTHER] != 0)
    {
      k_al_hamming<true><<<vsa_grid(waves), AL_BLOCK, 0, nullptr>>>(p);
      VSA_HIP(hipGetLastError());
    }
    tkernel.stop();
    if (exclusive_sum(p.cnt, offsets.as<uint64_t>(), n, nullptr, &words) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemcpy(cw, counters.p, sizeof cw, hipMemcpyDeviceToHost));
    if (cw[AL_NABOVE] != 0 || cw[AL_NOROOM] != 0)
    {
      VSA_ERROR("%s: the edit distance of %lu records is above the distance "
                "they carry (%lu scripts left their room)", who,
                (unsigned long) cw[AL_NABOVE], (unsigned long) cw[AL_NOROOM]);
      return -2;
    }
    if (cw[AL_NEDIST] == 0)
    {
      // every script fills its room: the array is tight as it is
      eops.p = tmp.release();
    } else
    {
      if (eops.alloc(words * 2) != 0)
      {
        return -100;
      }
      k_al_gather<<<vsa_grid((n + AL_BLOCK - 1) / AL_BLOCK), AL_BLOCK, 0,
                    nullptr>>>(p.tmp, p.tmpoff, offsets.as<uint64_t>(), n,
                               eops.as<uint16_t>());
      VSA_HIP(hipGetLastError());
    }
  }
  tall.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  vsa_alignments *a = new vsa_alignments;
  a->device = index->device;
  a->offsets = (uint64_t *) offsets.release();
  a->eops = (uint16_t *) eops.release();
  memset(&a->stats, 0, sizeof a->stats);
  a->stats.count = n;
  a->stats.words = words;
  a->stats.edist = cw[AL_NEDIST];
  a->stats.staged = cw[AL_NSTAGE];
  a->stats.kernel_ms = tkernel.ms();
  a->stats.total_device_ms = tall.ms();
  *alignments = a;
  return 0;
}

extern "C" int vsa_alignments_info(const vsa_alignments *a,
                                   vsa_alignstats *stats)
{
  if (a == nullptr || stats == nullptr)
  {
    VSA_ERROR("vsa_alignments_info: NULL argument");
    return -1;
  }
  *stats = a->stats;
  return 0;
}

extern "C" int vsa_alignments_fetch(const vsa_alignments *a, uint64_t *offsets,
                                    uint16_t *eops)
{
  if (a == nullptr)
  {
    VSA_ERROR("vsa_alignments_fetch: NULL argument");
    return -1;
  }
  if (enter(a->device) != 0)
  {
    return -100;
  }
  if (offsets != nullptr)
  {
    VSA_HIP(hipMemcpy(offsets, a->offsets, (a->stats.count + 1) * 8,
                      hipMemcpyDeviceToHost));
  }
  if (eops != nullptr && a->stats.words > 0)
  {
    VSA_HIP(hipMemcpy(eops, a->eops, a->stats.words * 2,
                      hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" void vsa_alignments_free(vsa_alignments *a)
{
  if (a == nullptr)
  {
    return;
  }
  (void) hipSetDevice(a->device);
  vsa_dev_free(a->offsets);
  vsa_dev_free(a->eops);
  delete a;
}
