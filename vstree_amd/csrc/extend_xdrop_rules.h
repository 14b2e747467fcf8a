/*
  The rules of the X-drop extension of exact seeds (vmatch -hxdrop X and
  -exdrop X with -l L), stated ONCE for the host (extend_xdrop_host.c) and for
  the kernels (extend_xdrop.hip): the seed length (Vmatch/matchlenparm.c:40-46),
  the two Hamming scans (evalhammingxdropleft / -right, kurtz/xdrop.c:37-140),
  the greedy generations of the edit extension (EVALXDROPEDIT, kurtz/xdrop.gen:
  2-201 with the macros of kurtz/xdrop.c:151-261) and what xdropseedextend
  (Vmengine/xdropext.c:39-221) makes of the two sides.  Plain C that both
  compilers read; integers only.

  One candidate per seed: nothing is chosen among extensions, so no E-value
  is read here.

  -hxdrop.  A side is a sequence of symbol pairs at t = 0, 1, .. from the
  symbol directly beside the seed (it IS compared, unlike in hammingextend);
  a match scores +2, a mismatch -1 (a wildcard never matches), a separator or
  the end of either array ends the side.  The side stops when the score falls
  below best - X, and best moves on a strict improvement only.  A run of
  matches can only raise the score, so however the symbols are read -- one by
  one, in words of 8, by a wavefront -- only the marks (mismatch, wildcard,
  separator) are events; the matches between two marks are applied as one
  run.  The left side rejects the SEED as soon as `reach` (the seed length
  parameter) matches in a row are seen: a longer exact seed covers it.

  -exdrop.  The generations of Zhang et al.: generation d holds, for every
  diagonal k = lower - 1 .. upper + 1, the furthest row i reached with d
  differences; an entry comes from its three predecessors (the order and the
  comparisons below are the reference's and decide ties), is pruned when its
  score lies below the best of (X + 1) / 3 generations ago minus X, slides
  along equal symbols, and the band of the next generation is what stayed
  finite and inside both arrays.  ulen and vlen are STATE: a slide that reads
  a separator shortens the array it read it in, for every later diagonal of
  the same and of all later generations, and on the left side, where symbol I
  is useq[ulen - 1 - I], the same I then addresses another symbol.
*/
#ifndef VSA_EXTEND_XDROP_RULES_H
#define VSA_EXTEND_XDROP_RULES_H
#include <stdint.h>
#include "vstree_amd.h"
#include "extend_rules.h"

/* Matchparam.seedlength with an X-drop option, Vmatch/matchlenparm.c:40-46:
   -seedlength S, or DEFAULTSEEDLENGTH; not max(S, L / (K + 1)) */
VSA_HD uint64_t vsa_xd_seedlength(uint64_t seedlength)
{
  return seedlength == 0 ? 30 : seedlength;
}

/* Xdropbest */
typedef struct
{
  int64_t ivalue, jvalue, score;
} vsa_xd_best;

/* ---- -hxdrop: one side in the making --------------------------------- */

typedef struct
{
  int64_t total, best, xdrop;
  uint64_t bestlen; /* symbols up to the best score                      */
  uint64_t done;    /* pairs looked at: all before `done` were matches
                       since the last event                               */
  uint64_t run;     /* matches in a row (the left side)                   */
  uint64_t reach;
  int left;
} vsa_xd_scan;

VSA_HD void vsa_xd_begin(vsa_xd_scan *s, uint64_t xdrop, uint64_t reach,
                         int left)
{
  s->total = s->best = 0;
  s->xdrop = (int64_t) xdrop;
  s->bestlen = s->done = s->run = 0;
  s->reach = reach;
  s->left = left;
}

#define VSA_XD_ON 0     /* the side goes on                               */
#define VSA_XD_OVER 1   /* ... is over                                    */
#define VSA_XD_REJECT 2 /* the seed is rejected (xdrop.c:121-124)         */

/* the pairs done .. t - 1 match */
VSA_HD int vsa_xd_matches(vsa_xd_scan *s, uint64_t t)
{
  const uint64_t r = t - s->done;

  if (r == 0)
  {
    return VSA_XD_ON;
  }
  s->done = t;
  if (s->left)
  {
    s->run += r;
    if (s->run >= s->reach)
    {
      return VSA_XD_REJECT;
    }
  }
  /* the score rises with every pair: the drop test holds throughout, and
     the last pair of the run is the best one if any is */
  s->total += 2 * (int64_t) r;
  if (s->best < s->total)
  {
    s->best = s->total;
    s->bestlen = t;
  }
  return VSA_XD_ON;
}

/* a mismatch at pair t, behind matches */
VSA_HD int vsa_xd_mismatch(vsa_xd_scan *s, uint64_t t)
{
  const int rc = vsa_xd_matches(s, t);

  if (rc != VSA_XD_ON)
  {
    return rc;
  }
  s->run = 0;
  s->done = t + 1;
  s->total -= 1;
  return s->total < s->best - s->xdrop ? VSA_XD_OVER : VSA_XD_ON;
}

/* a separator at pair t, or the end of an array in front of it */
VSA_HD int vsa_xd_end(vsa_xd_scan *s, uint64_t t)
{
  const int rc = vsa_xd_matches(s, t);

  return rc == VSA_XD_REJECT ? rc : VSA_XD_OVER;
}

/* where a side lies: pair t is p1[-t], p2[-t] (left) or p1[t], p2[t], for
   t < nsym; 0 pairs where an array ends beside the seed */
typedef struct
{
  const uint8_t *p1, *p2;
  uint64_t nsym;
} vsa_xd_plan;

VSA_HD void vsa_xd_prepare(const vsa_ext_view *v1, uint64_t pos1,
                           const vsa_ext_view *v2, uint64_t pos2,
                           uint64_t length, int left, vsa_xd_plan *plan)
{
  if (left)
  {
    /* the arrays of xdropext.c:74-80 run to position 0 of the Multiseq; a
       view that does not begin it has a separator in front, which ends the
       side like the end of the array */
    plan->p1 = v1->p + pos1 - 1;
    plan->p2 = v2->p + pos2 - 1;
    plan->nsym = pos1 < pos2 ? pos1 : pos2;
  } else
  {
    const uint64_t r1 = v1->len - (pos1 + length),
                   r2 = v2->len - (pos2 + length);
    plan->p1 = v1->p + pos1 + length;
    plan->p2 = v2->p + pos2 + length;
    plan->nsym = r1 < r2 ? r1 : r2;
  }
}

/* the events of the marks of one word whose first pair is t0 (marks of
   pairs at or behind nsym do not count) */
VSA_HD int vsa_xd_events(vsa_xd_scan *s, const vsa_xd_plan *plan, uint64_t t0,
                         uint32_t marks, uint32_t sep)
{
  uint32_t k;

  for (k = 0; marks >> k != 0; k++)
  {
    if (marks >> k & 1u)
    {
      int rc;
      if (t0 + k >= plan->nsym)
      {
        return VSA_XD_ON;
      }
      rc = (sep >> k & 1u) ? vsa_xd_end(s, t0 + k)
                           : vsa_xd_mismatch(s, t0 + k);
      if (rc != VSA_XD_ON)
      {
        return rc;
      }
    }
  }
  return VSA_XD_ON;
}

/* no mark among the pairs in front of t: they match.  Called behind the
   events of every word, so that the left side rejects its seed within a word
   (a step of the wavefront) of the pair the reference rejects it at. */
VSA_HD int vsa_xd_upto(vsa_xd_scan *s, const vsa_xd_plan *plan, uint64_t t)
{
  return vsa_xd_matches(s, t < plan->nsym ? t : plan->nsym);
}

/* the event behind the last pair of the plan */
VSA_HD int vsa_xd_finishside(vsa_xd_scan *s, const vsa_xd_plan *plan)
{
  return vsa_xd_end(s, plan->nsym);
}

VSA_HD void vsa_xd_scanbest(const vsa_xd_scan *s, vsa_xd_best *b)
{
  b->ivalue = b->jvalue = (int64_t) s->bestlen;
  b->score = s->best;
}

/* ---- -exdrop: EVALXDROPEDIT -------------------------------------------- */

/* the two arrays of a side and their lengths, which the slides change */
typedef struct
{
  const uint8_t *useq, *vseq;
  int64_t ulen, vlen;
  int left;
} vsa_xd_arrays;

/* The arrays of a side of a seed of `length` symbols at pos1 of seq1[0 .. n1)
   and pos2 of seq2[0 .. n2), the two Multiseqs: to the left everything in
   front of the seed, to the right everything behind it, whatever sequences
   that spans.  0: the side is not extended, a neighbour of the seed is a
   separator or a Multiseq ends there (xdropext.c:94-101,123-130). */
VSA_HD int vsa_xd_arrays_init(vsa_xd_arrays *a, const uint8_t *seq1,
                              uint64_t n1, const uint8_t *seq2, uint64_t n2,
                              uint64_t pos1, uint64_t pos2, uint64_t length,
                              int left)
{
  a->left = left;
  if (left)
  {
    if (pos1 == 0 || seq1[pos1 - 1] == (uint8_t) VSA_SEPARATOR || pos2 == 0 ||
        seq2[pos2 - 1] == (uint8_t) VSA_SEPARATOR)
    {
      return 0;
    }
    a->useq = seq1;
    a->ulen = (int64_t) pos1;
    a->vseq = seq2;
    a->vlen = (int64_t) pos2;
  } else
  {
    if (pos1 + length >= n1 ||
        seq1[pos1 + length] == (uint8_t) VSA_SEPARATOR ||
        pos2 + length >= n2 ||
        seq2[pos2 + length] == (uint8_t) VSA_SEPARATOR)
    {
      return 0;
    }
    a->useq = seq1 + pos1 + length;
    a->ulen = (int64_t) (n1 - (pos1 + length));
    a->vseq = seq2 + pos2 + length;
    a->vlen = (int64_t) (n2 - (pos2 + length));
  }
  return 1;
}

/* USEQ / VSEQ, xdrop.c:239-240,258-259 */
VSA_HD uint8_t vsa_xd_usym(const vsa_xd_arrays *a, int64_t i)
{
  return a->left ? a->useq[a->ulen - 1 - i] : a->useq[i];
}

VSA_HD uint8_t vsa_xd_vsym(const vsa_xd_arrays *a, int64_t j)
{
  return a->left ? a->vseq[a->vlen - 1 - j] : a->vseq[j];
}

/* COMPARESYMBOLSSEP(i, j) for i < ulen, j < vlen: 1 the symbols match, 0
   they end the slide -- a separator shortens its array */
VSA_HD int vsa_xd_compare(vsa_xd_arrays *a, int64_t i, int64_t j)
{
  const uint8_t x = vsa_xd_usym(a, i);
  uint8_t y;

  if (x == (uint8_t) VSA_SEPARATOR)
  {
    a->ulen = i;
    return 0;
  }
  y = vsa_xd_vsym(a, j);
  if (y == (uint8_t) VSA_SEPARATOR)
  {
    a->vlen = j;
    return 0;
  }
  return !(x != y || x == (uint8_t) VSA_WILDCARD);
}

/* the slide of xdrop.gen:122-135 from (*i, *j); bytewise: one symbol per
   step, else the marks of words of 8 find the pair that ends it */
VSA_HD void vsa_xd_slide(vsa_xd_arrays *a, int64_t *i, int64_t *j,
                         int bytewise)
{
  while (*i < a->ulen && *j < a->vlen)
  {
    if (!bytewise)
    {
      const int64_t ru = a->ulen - *i, rv = a->vlen - *j;
      const uint64_t valid = (uint64_t) (ru < rv ? ru : rv);
      const uint8_t *pu = a->left ? a->useq + (a->ulen - 1 - *i)
                                  : a->useq + *i,
                    *pv = a->left ? a->vseq + (a->vlen - 1 - *j)
                                  : a->vseq + *j;
      uint32_t sep, marks;

      marks = vsa_ext_marks8(vsa_ext_word(pu, a->left, 0, valid),
                             vsa_ext_word(pv, a->left, 0, valid), &sep);
      if (valid < 8)
      {
        marks &= (1u << valid) - 1u;
      }
      if (marks == 0)
      {
        *i += valid < 8 ? (int64_t) valid : 8;
        *j += valid < 8 ? (int64_t) valid : 8;
        continue;
      }
      while ((marks & 1u) == 0)
      {
        marks >>= 1;
        (*i)++;
        (*j)++;
      }
    }
    if (!vsa_xd_compare(a, *i, *j))
    {
      return;
    }
    (*i)++;
    (*j)++;
  }
}

/* dback of generation 1, xdrop.gen:7-8: C division */
VSA_HD int64_t vsa_xd_dback(int64_t xdrop)
{
  return -(xdrop + 1) / 3;
}

/* the T values of the last VSA_XD_RING generations: the test of generation
   d reads the one of generation d - 1 - (X + 1) / 3, at most 86 back */
#define VSA_XD_RING 128

/* TTAB(D) */
VSA_HD int64_t vsa_xd_ttab(const int64_t *ring, int64_t d, int64_t xdrop)
{
  return d < 0 ? -xdrop : ring[d & (VSA_XD_RING - 1)];
}

/* row i of diagonal k from the previous generation (pm1, p0, pp1: its rows
   on k - 1, k, k + 1; minf: minus infinity), xdrop.gen:85-109 */
VSA_HD int64_t vsa_xd_entry(int64_t k, int64_t lower, int64_t upper,
                            int64_t pm1, int64_t p0, int64_t pp1,
                            int64_t minf)
{
  int64_t i = minf;

  if (k < upper && pp1 != minf && i < pp1) /* insertion */
  {
    i = pp1;
  }
  if (lower <= k && k <= upper && p0 != minf && i <= p0) /* mismatch */
  {
    i = p0 + 1;
  }
  if (lower < k && pm1 != minf && i <= pm1) /* deletion */
  {
    i = pm1 + 1;
  }
  return i;
}

/* SPRIME(i + j) under dmulti = 3 d */
VSA_HD int64_t vsa_xd_sprime(int64_t i, int64_t j, int64_t dmulti)
{
  return (i + j) - dmulti;
}

/* what a generation leaves for the band of the next one */
typedef struct
{
  int64_t minisfinite, maxisfinite, maxisN, minisM;
} vsa_xd_band;

VSA_HD void vsa_xd_band_begin(vsa_xd_band *b, int64_t integermax)
{
  b->minisfinite = b->minisM = integermax;
  b->maxisfinite = b->maxisN = -integermax;
}

/* diagonal k ended its slide at (i, j), xdrop.gen:136-148; in ascending k */
VSA_HD void vsa_xd_band_note(vsa_xd_band *b, const vsa_xd_arrays *a, int64_t k,
                             int64_t i, int64_t j)
{
  if (j == a->vlen)
  {
    b->maxisN = k;
  }
  if (i == a->ulen && b->minisM > k)
  {
    b->minisM = k;
  }
  if (b->minisfinite > k)
  {
    b->minisfinite = k;
  }
  b->maxisfinite = k;
}

/* xdrop.gen:160-177; 1: the side is over.  A generation without a finite
   entry ends the side too.  Where both arrays have 2 symbols or more that is
   what lower > upper + 2 says already (lower = integermax, upper =
   -integermax); with arrays of one symbol it says 1 > 1, and the reference
   goes on making empty generations until its memory is used up.  Maximal
   seeds never get there (the symbol beside them is a mismatch, and the
   generation behind it ends at both array ends). */
VSA_HD int vsa_xd_band_next(const vsa_xd_band *b, int64_t *lower,
                            int64_t *upper)
{
  *lower = b->minisfinite > b->maxisN + 2 ? b->minisfinite : b->maxisN + 2;
  *upper = b->maxisfinite < b->minisM - 2 ? b->maxisfinite : b->minisM - 2;
  return *lower > *upper + 2 || b->maxisfinite < b->minisfinite;
}

/* bestscore < tmpscore, strict: the first of equal maxima stays */
VSA_HD void vsa_xd_better(vsa_xd_best *best, int64_t i, int64_t j,
                          int64_t score)
{
  if (best->score < score)
  {
    best->score = score;
    best->ivalue = i;
    best->jvalue = j;
  }
}

/* One side by the generations above, diagonal by diagonal in the reference's
   order.  g0, g1: two rows of `cap` entries for the generations; ring:
   VSA_XD_RING entries.  0 and *best, or 1: a generation is wider than cap
   (nothing of *best holds; the caller comes again with wider rows). */
VSA_HD int vsa_xd_editside(vsa_xd_arrays *a, int64_t xdrop, int64_t *g0,
                           int64_t *g1, int64_t cap, int64_t *ring,
                           int bytewise, vsa_xd_best *best)
{
  const int64_t integermax = a->ulen > a->vlen ? a->ulen : a->vlen,
                minf = -integermax;
  int64_t *cur = g0, *prev = g1, prevsmallest = 0, dback = vsa_xd_dback(xdrop),
          dmulti = 0, d = 1, lower = 0, upper = 0, i = 0, j = 0, k;

  if (cap < 3)
  {
    return 1;
  }
  /* (the loop of xdrop.gen:30-33 is a slide from (0, 0)) */
  vsa_xd_slide(a, &i, &j, bytewise);
  cur[0] = i;
  best->score = i + i;
  best->ivalue = best->jvalue = i;
  ring[0] = best->score - xdrop;
  for (;;)
  {
    vsa_xd_band band;
    int64_t *t = cur, dbackvalue;

    if (upper - lower + 3 > cap)
    {
      return 1;
    }
    dmulti += 3;
    cur = prev;
    prev = t;
    vsa_xd_band_begin(&band, integermax);
    dbackvalue = vsa_xd_ttab(ring, dback, xdrop);
    for (k = lower - 1; k <= upper + 1; k++)
    {
      /* (a row outside lower - 1 .. upper + 1 of the previous generation is
         not read: the three tests of vsa_xd_entry keep it out) */
      const int64_t at = k - prevsmallest;
      const int64_t pm1 = lower < k ? prev[at - 1] : minf,
                    p0 = (lower <= k && k <= upper) ? prev[at] : minf,
                    pp1 = k < upper ? prev[at + 1] : minf;

      i = vsa_xd_entry(k, lower, upper, pm1, p0, pp1, minf);
      if (i != minf)
      {
        j = i - k;
        if (vsa_xd_sprime(i, j, dmulti) < dbackvalue)
        {
          i = minf;
        } else
        {
          vsa_xd_slide(a, &i, &j, bytewise);
          vsa_xd_band_note(&band, a, k, i, j);
          vsa_xd_better(best, i, j, vsa_xd_sprime(i, j, dmulti));
        }
      }
      cur[k - (lower - 1)] = i;
    }
    prevsmallest = lower - 1;
    if (vsa_xd_band_next(&band, &lower, &upper))
    {
      return 0;
    }
    ring[d & (VSA_XD_RING - 1)] = best->score - xdrop;
    d++;
    dback++;
  }
}

/* ---- both sides together, xdropext.c:164-219 ----------------------------- */

/* acceptmatch, xdropext.c:21-37 */
VSA_HD int vsa_xd_accept(uint64_t length1, uint64_t pos1, uint64_t length2,
                         uint64_t pos2)
{
  if (pos1 >= pos2)
  {
    return 0;
  }
  if (pos1 + length1 - 1 < pos2)
  {
    return 1;
  }
  if (pos1 + length1 >= pos2 + length2)
  {
    return 0;
  }
  return 1;
}

/* EVALSCORE2DISTANCE, include/match.h:76-77: C division */
VSA_HD int64_t vsa_xd_distance(int64_t score, uint64_t length1,
                               uint64_t length2)
{
  const int64_t sum = (int64_t) (length1 + length2);

  return score >= 0 ? (sum - score) / 3 : -((sum + score) / 3);
}

typedef struct
{
  uint64_t pos1, pos2, length1, length2;
  int64_t distance; /* negative for -hxdrop */
} vsa_xd_match;

/* A seed of `length` symbols at seed1 of seq1 and seed2 of seq2 with its two
   sides.  self: neither rcmode nor querycompare (the swap and acceptmatch
   apply).  1 and *m -- matchokay (Vmatch/mokay.c:16-24) included --, or 0. */
VSA_HD int vsa_xd_finish(const uint8_t *seq1, const uint8_t *seq2, int self,
                         int hamming, uint64_t seed1, uint64_t seed2,
                         uint64_t length, const vsa_xd_best *l,
                         const vsa_xd_best *r, uint64_t leastlength,
                         vsa_xd_match *m)
{
  uint64_t pos1 = seed1 - (uint64_t) l->ivalue,
           pos2 = seed2 - (uint64_t) l->jvalue, length1, length2;
  const int64_t exti = l->ivalue + r->ivalue, extj = l->jvalue + r->jvalue;
  int64_t score;

  if (!self || pos1 <= pos2)
  {
    length1 = length + (uint64_t) exti;
    length2 = length + (uint64_t) extj;
  } else
  {
    const uint64_t temp = pos1;
    pos1 = pos2;
    pos2 = temp;
    length1 = length + (uint64_t) extj;
    length2 = length + (uint64_t) exti;
  }
  if (seq1[pos1 + length1 - 1] == (uint8_t) VSA_SEPARATOR)
  {
    length1--;
  }
  if (seq1[pos1] == (uint8_t) VSA_SEPARATOR)
  {
    pos1++;
    length1--;
  }
  if (seq2[pos2 + length2 - 1] == (uint8_t) VSA_SEPARATOR)
  {
    length2--;
  }
  if (seq2[pos2] == (uint8_t) VSA_SEPARATOR)
  {
    pos2++;
    length2--;
  }
  if (self && !vsa_xd_accept(length1, pos1, length2, pos2))
  {
    return 0;
  }
  score = l->score + r->score + 2 * (int64_t) length;
  if (hamming)
  {
    score = -score;
  }
  m->distance = vsa_xd_distance(score, length1, length2);
  m->pos1 = pos1;
  m->pos2 = pos2;
  m->length1 = length1;
  m->length2 = length2;
  return length1 >= leastlength && length2 >= leastlength;
}

/* the record of a match: seed2 the place of the seed in seq2 (queries: in
   the batch's Multiseq or in its sequence, as pos2 is) */
VSA_HD void vsa_xd_record(const vsa_match *seed, int self, uint64_t seed2,
                          const vsa_xd_match *m, vsa_match *out)
{
  const uint64_t dist = (uint64_t) (m->distance < 0 ? -m->distance
                                                    : m->distance);

  out->length = VSA_XDROP_PACKLENGTHS(m->length1, m->length2);
  out->dbstart = m->pos1;
  if (self)
  {
    out->queryseq = m->pos2;
    out->querystart = VSA_XDROP_PACKSTART(0, dist);
  } else
  {
    /* relpos2 = seed->relpos2 - (seed->position2 - pos2) */
    out->queryseq = seed->queryseq;
    out->querystart =
        VSA_XDROP_PACKSTART(seed->querystart - (seed2 - m->pos2), dist);
  }
}

#endif
