/*
  The rules of the edit-distance extension of exact seeds (vmatch -l L -e K
  outside -complete), stated ONCE for the host (extend_edist_host.c) and for
  the kernels (extend_edist.hip): editextend (kurtz/extendED.c:78-355) with
  acceptmatch (:24-48), the greedy fronts of extendedleftSEP / extendedrightSEP
  (kurtz/frontSEP.c:65-339) over the front functions of kurtz/front.gen:48-182,
  and cmpmatches (include/extcmp.c).  Plain C that both compilers read; the
  double operations are table reads, one multiplication and one division per
  candidate, in the reference's order, so host and device agree bit for bit.

  Both Multiseqs are FLAT here: all sequences of the index, or of the query
  batch, in one array with a separator between two of them, as the reference
  holds them.  The views of extend_rules.h (one query sequence with a
  separator supplied around it) are not enough for this extension, because
  the literal order of the reference can step over a separator nobody has
  looked at (below), and then the symbols of the neighbouring sequence are
  read.

  A SIDE of a seed is the pair of texts u, v that begin beside it and run to
  the end of their Multiseq (right side) or back to its start (left side);
  offset d of a side is the d-th symbol away from the seed, whichever way
  that is in memory.  ulen / vlen are the lengths of these rests, so a seed
  within K symbols of either end of a Multiseq has narrower fronts
  (frontspecparms with r = p - min(ulen, vlen) > 0).

  Front p holds a row for every diagonal k = -p .. p: the row t of u reached
  with p errors where v is at t + k.  An entry is made of three entries of
  front p - 1 (vsa_er_best), then slid along equal symbols (a special symbol
  equals nothing).  What is particular to the reference and kept literally:

    bounds    ubound / vbound start at the end of the rest, or at a separator
              among the first K + 1 (right) or K (left) symbols, and MOVE
              whenever a slide reads a separator (COMPARESYMBOLS).  Within a
              front the diagonals are evaluated in ascending order, and each
              sees the bounds as the ones before it left them.  "The first
              separator of the side" is NOT an equivalent bound: a slide that
              stops because u is at its bound has not read v's symbol there,
              and if that symbol is a separator beyond the pre-scanned window
              the next diagonal steps over it (entry from below, the row
              stands and v advances by one).  vsa_ed_replay gives a slide made
              under the bounds of the start of the front the outcome it has
              under the bounds of its turn, so that lanes may slide at once.
    MINUSINFINITYFRONT is -max(ulen, vlen), a number that takes part in the
              maximum: with max(ulen, vlen) = 1 it is -1 and "-1 + 1" is a
              row.
    same text a diagonal on which u and v are the same place of one array
              (self seeds less than K apart) is not slid along; its row
              becomes ulen - 1 (front.gen:120-123, frontSEP.c:105-108).
    stop rule on the left only, a slide over >= seedlength symbols makes the
              entry undefined and ends the side with this front
              (frontSEP.c:120-128, 327-334).
*/
#ifndef VSA_EXTEND_EDIST_RULES_H
#define VSA_EXTEND_EDIST_RULES_H
#include <stdint.h>
#include "vstree_amd.h"
#include "extend_rules.h"
#include "erate_rules.h"

#ifndef VSA_ED_ROW
#define VSA_ED_ROW uint64_t /* a stored entry of a front */
#endif
#define VSA_ED_UNDEF ((VSA_ED_ROW) ~(VSA_ED_ROW) 0)
#define VSA_ED_NOSAME INT64_MIN

/* entries of the fronts 0 .. maxdist of one side; entry (p, k) at
   [p * p + k + p] */
VSA_HD uint64_t vsa_ed_frontwords(uint64_t maxdist)
{
  return (maxdist + 1) * (maxdist + 1);
}

VSA_HD uint64_t vsa_ed_at(int64_t p, int64_t k)
{
  return (uint64_t) (p * p + k + p);
}

typedef struct
{
  const uint8_t *s1, *s2; /* the two Multiseqs                               */
  int64_t o1, o2;         /* the places of the symbols at offset 0           */
  int64_t ulen, vlen;     /* symbols from there to the end of the Multiseq   */
  int64_t neg;            /* MINUSINFINITYFRONT                              */
  int64_t samediag;       /* the diagonal of the same text, VSA_ED_NOSAME    */
  int64_t maxdist;
  uint64_t reach;         /* the seed length of the stop rule                */
  int left;
} vsa_ed_side;

typedef struct
{
  int64_t ub, vb; /* offsets the slides stay below */
} vsa_ed_bounds;

VSA_HD uint8_t vsa_ed_symu(const vsa_ed_side *s, int64_t d)
{
  return s->s1[s->left ? s->o1 - d : s->o1 + d];
}

VSA_HD uint8_t vsa_ed_symv(const vsa_ed_side *s, int64_t d)
{
  return s->s2[s->left ? s->o2 - d : s->o2 + d];
}

/* one side of a seed of `length` symbols at pos1 of s1[0 .. n1) and pos2 of
   s2[0 .. n2), which it fits; self: both are the same array
   (extendED.c:116-132, frontSEP.c:225-229, 308-312) */
VSA_HD void vsa_ed_side_init(vsa_ed_side *s, const uint8_t *s1, uint64_t n1,
                             const uint8_t *s2, uint64_t n2, int self,
                             uint64_t pos1, uint64_t pos2, uint64_t length,
                             int left, uint64_t maxdist, uint64_t seedlength)
{
  s->s1 = s1;
  s->s2 = s2;
  s->left = left;
  s->maxdist = (int64_t) maxdist;
  s->reach = seedlength;
  if (left)
  {
    s->o1 = (int64_t) pos1 - 1;
    s->o2 = (int64_t) pos2 - 1;
    s->ulen = (int64_t) pos1;
    s->vlen = (int64_t) pos2;
    s->samediag = self ? (int64_t) pos2 - (int64_t) pos1 : VSA_ED_NOSAME;
  } else
  {
    s->o1 = (int64_t) (pos1 + length);
    s->o2 = (int64_t) (pos2 + length);
    s->ulen = (int64_t) n1 - s->o1;
    s->vlen = (int64_t) n2 - s->o2;
    s->samediag = self ? (int64_t) pos1 - (int64_t) pos2 : VSA_ED_NOSAME;
  }
  s->neg = -(s->ulen > s->vlen ? s->ulen : s->vlen);
}

/* the bounds before the first front: a separator among the first maxdist + 1
   symbols of a right side, the first maxdist of a left side
   (frontSEP.c:207-224, 276-307) */
VSA_HD void vsa_ed_bounds_init(const vsa_ed_side *s, vsa_ed_bounds *b)
{
  const int64_t window = s->left ? s->maxdist : s->maxdist + 1;
  int64_t d;

  b->ub = s->ulen;
  for (d = 0; d < window && d < s->ulen; d++)
  {
    if (vsa_ed_symu(s, d) == VSA_SEPARATOR)
    {
      b->ub = d;
      break;
    }
  }
  b->vb = s->vlen;
  for (d = 0; d < window && d < s->vlen; d++)
  {
    if (vsa_ed_symv(s, d) == VSA_SEPARATOR)
    {
      b->vb = d;
      break;
    }
  }
}

/* no front but front 0 is made (frontSEP.c:234, 317) */
VSA_HD int vsa_ed_bothempty(const vsa_ed_side *s)
{
  return s->ulen == s->vlen && s->vlen == 0;
}

/* the diagonals lo .. hi front p stores (frontspecparms, front.gen:48-63) */
VSA_HD void vsa_ed_range(const vsa_ed_side *s, int64_t p, int64_t *lo,
                         int64_t *hi)
{
  const int64_t r = p - (s->ulen < s->vlen ? s->ulen : s->vlen);

  if (r <= 0)
  {
    *lo = -p;
    *hi = p;
  } else
  {
    *lo = -s->ulen > -p ? -s->ulen : -p;
    *hi = s->vlen < p ? s->vlen : p;
  }
}

/* entry (p, k) is evaluated; every other one is undefined (front.gen:65-72,
   162, frontSEP.c:156) */
VSA_HD int vsa_ed_evaluated(const vsa_ed_side *s, int64_t p, int64_t k)
{
  const int64_t r = p - (s->ulen < s->vlen ? s->ulen : s->vlen);
  int64_t lo, hi;

  vsa_ed_range(s, p, &lo, &hi);
  return k >= lo && k <= hi && (r <= 0 || k <= -r || k >= r);
}

#define VSA_ED_NONE 0  /* the entry is undefined                             */
#define VSA_ED_FIXED 1 /* *t is the row, nothing is slid along               */
#define VSA_ED_SLIDE 2 /* the row is *t plus what a slide from there matches */

/* an entry from its three predecessors, undefined ones given as s->neg
   (front.gen:90-123, frontSEP.c:77-108) */
VSA_HD int vsa_ed_start(const vsa_ed_side *s, int64_t same, int64_t below,
                        int64_t above, int64_t k, int64_t *t)
{
  *t = vsa_er_best(same, below, above);
  if (*t < 0 || *t + k < 0)
  {
    return VSA_ED_NONE;
  }
  if (s->ulen == 0 || s->vlen == 0)
  {
    return VSA_ED_FIXED;
  }
  if (k == s->samediag)
  {
    *t = s->ulen - 1;
    return VSA_ED_FIXED;
  }
  return VSA_ED_SLIDE;
}

/* the symbols u[t ..) and v[t + k ..) agree in below the bounds, one at a
   time; a separator that is read moves its bound (COMPARESYMBOLS,
   frontSEP.c:27-39) */
VSA_HD int64_t vsa_ed_slide(const vsa_ed_side *s, int64_t t, int64_t k,
                            vsa_ed_bounds *b)
{
  int64_t m = 0;

  while (t + m < b->ub && t + m + k < b->vb)
  {
    const uint8_t a = vsa_ed_symu(s, t + m), c = vsa_ed_symv(s, t + m + k);
    if (a == VSA_SEPARATOR)
    {
      b->ub = t + m;
    }
    if (c == VSA_SEPARATOR)
    {
      b->vb = t + m + k;
    }
    if (a != c || VSA_ER_ISSPECIAL(a))
    {
      break;
    }
    m++;
  }
  return m;
}

/* the first mark of a pair of words -> what the read of that symbol pair
   does to the bounds: bit 0 u's symbol is a separator, bit 1 v's */
VSA_HD int vsa_ed_seps(uint64_t a, uint64_t c, uint32_t j)
{
  return ((uint8_t) (a >> (8 * j)) == VSA_SEPARATOR ? 1 : 0) |
         ((uint8_t) (c >> (8 * j)) == VSA_SEPARATOR ? 2 : 0);
}

/* the same slide eight symbols per step (vsa_ext_word, vsa_ext_marks8) */
VSA_HD int64_t vsa_ed_slide8(const vsa_ed_side *s, int64_t t, int64_t k,
                             vsa_ed_bounds *b)
{
  const int64_t ru = b->ub - t, rv = b->vb - (t + k);
  const int64_t rem = ru < rv ? ru : rv;
  const uint8_t *pu, *pv;
  int64_t m = 0;

  if (rem <= 0)
  {
    return 0;
  }
  pu = s->s1 + (s->left ? s->o1 - t : s->o1 + t);
  pv = s->s2 + (s->left ? s->o2 - (t + k) : s->o2 + (t + k));
  while (m < rem)
  {
    const uint64_t valid = (uint64_t) (rem - m);
    const uint64_t a = vsa_ext_word(pu, s->left, (uint64_t) m, valid),
                   c = vsa_ext_word(pv, s->left, (uint64_t) m, valid);
    uint32_t sep;
    uint32_t marks = vsa_ext_marks8(a, c, &sep);

    if (valid < 8)
    {
      marks &= (1u << valid) - 1u;
    }
    if (marks != 0)
    {
      const uint32_t j = (uint32_t) __builtin_ctz(marks);
      const int seps = vsa_ed_seps(a, c, j);
      m += j;
      if (seps & 1)
      {
        b->ub = t + m;
      }
      if (seps & 2)
      {
        b->vb = t + m + k;
      }
      return m;
    }
    m += valid < 8 ? (int64_t) valid : 8;
  }
  return rem;
}

/* A slide from (t, t + k) made under bounds no tighter than *b matched m
   symbols and then, if `read`, read a pair of symbols with the separators
   `seps` (vsa_ed_seps).  -> what the same slide matches under *b, which it
   moves as that slide would: under tighter bounds it ends earlier and reads
   no pair. */
VSA_HD int64_t vsa_ed_replay(int64_t t, int64_t k, int64_t m, int read,
                             int seps, vsa_ed_bounds *b)
{
  const int64_t ru = b->ub - t, rv = b->vb - (t + k);
  const int64_t limit = ru < rv ? ru : rv;

  if (limit <= m)
  {
    return limit > 0 ? limit : 0;
  }
  if (read)
  {
    if (seps & 1)
    {
      b->ub = t + m;
    }
    if (seps & 2)
    {
      b->vb = t + m + k;
    }
  }
  return m;
}

/* what the front stores for an entry of `kind` with row t and a slide over
   m symbols, under the bounds as they stand behind that slide
   (front.gen:135-141, frontSEP.c:119-136); s->neg: undefined */
VSA_HD int64_t vsa_ed_stored(const vsa_ed_side *s, int kind, int64_t t,
                             int64_t m, int64_t k, const vsa_ed_bounds *b,
                             int *foundseed)
{
  if (kind == VSA_ED_NONE)
  {
    return s->neg;
  }
  if (kind == VSA_ED_SLIDE)
  {
    if (s->left && (uint64_t) m >= s->reach)
    {
      *foundseed = 1;
      return s->neg;
    }
    t += m;
  }
  return (t > b->ub || t + k > b->vb) ? s->neg : t;
}

/* after front p: 1 the side ends, with *h fronts beyond front 0
   (frontSEP.c:242-247, 327-336) */
VSA_HD int vsa_ed_frontends(const vsa_ed_side *s, int64_t p, int defined,
                            int foundseed, uint32_t *h)
{
  if (s->left && defined && foundseed)
  {
    *h = (uint32_t) p;
    return 1;
  }
  if (!defined)
  {
    *h = (uint32_t) (p - 1);
    return 1;
  }
  *h = (uint32_t) p;
  return p == s->maxdist;
}

VSA_HD int64_t vsa_ed_get(const vsa_ed_side *s, const VSA_ED_ROW *front,
                          int64_t p, int64_t k)
{
  if (k < -p || k > p)
  {
    return s->neg;
  }
  return front[k + p] == VSA_ED_UNDEF ? s->neg : (int64_t) front[k + p];
}

/* all fronts of a side, the diagonals of a front in ascending order, into
   fronts[vsa_ed_frontwords(maxdist)] -> the number of the last front the
   choice looks at (extendedrightSEP, extendedleftSEP).  bytewise: slide one
   symbol at a time. */
VSA_HD uint32_t vsa_ed_fronts(const vsa_ed_side *s, VSA_ED_ROW *fronts,
                              int bytewise)
{
  vsa_ed_bounds b;
  int foundseed = 0;
  uint32_t h = 0;
  int64_t p, k;

  vsa_ed_bounds_init(s, &b);
  fronts[0] = 0;
  if (vsa_ed_bothempty(s))
  {
    return 0;
  }
  for (p = 1; p <= s->maxdist; p++)
  {
    const VSA_ED_ROW *prev = fronts + vsa_ed_at(p - 1, -(p - 1));
    VSA_ED_ROW *cur = fronts + vsa_ed_at(p, -p);
    int defined = 0;

    for (k = -p; k <= p; k++)
    {
      int64_t t = 0, m = 0, value = s->neg;
      if (vsa_ed_evaluated(s, p, k))
      {
        const int kind = vsa_ed_start(s, vsa_ed_get(s, prev, p - 1, k),
                                      vsa_ed_get(s, prev, p - 1, k - 1),
                                      vsa_ed_get(s, prev, p - 1, k + 1), k,
                                      &t);
        if (kind == VSA_ED_SLIDE)
        {
          m = bytewise ? vsa_ed_slide(s, t, k, &b)
                       : vsa_ed_slide8(s, t, k, &b);
        }
        value = vsa_ed_stored(s, kind, t, m, k, &b, &foundseed);
      }
      cur[k + p] = value < 0 ? VSA_ED_UNDEF : (VSA_ED_ROW) value;
      defined = defined || value >= 0;
    }
    if (vsa_ed_frontends(s, p, defined, foundseed, &h))
    {
      return h;
    }
  }
  return h;
}

/* ---- the choice, extendED.c:133-342 ---------------------------------------- */

typedef struct
{
  uint64_t pos1, pos2, length1, length2, dist;
} vsa_ed_match;

/* acceptmatch, extendED.c:24-48 */
VSA_HD int vsa_ed_accept(uint64_t dist, uint64_t length1, uint64_t pos1,
                         uint64_t length2, uint64_t pos2)
{
  if (pos1 >= pos2)
  {
    return 0;
  }
  if (pos1 + length1 - 1 < pos2) /* no overlap */
  {
    return 1;
  }
  if (pos1 + length1 >= pos2 + length2) /* embedded */
  {
    return 0;
  }
  /* the part that does not overlap is too small */
  return (pos2 - pos1) + (pos2 + length2) - (pos1 + length1) > dist;
}

/* cmpmatches (include/extcmp.c) with incgetEvalue(evalues, 1.0, dist, length)
   of an edit distance (kurtz/evalues.c:382-420): ev->hequot[dist] is the
   factor of that distance, 0.0 beyond VSA_EVALUES_MAXEDIST.  A tie answers
   1, so the later candidate wins. */
VSA_HD int vsa_ed_cmp(const vsa_selrules *ev, uint64_t dist1, uint64_t dist2,
                      uint64_t length1, uint64_t length2)
{
  double e1 = 0.0, e2 = 0.0, q1, q2, id1, id2;

  if (!ev->noevalue)
  {
    const double t1 = vsa_sel_lookup(ev, (int64_t) dist1, length1),
                 t2 = vsa_sel_lookup(ev, (int64_t) dist2, length2);
    if (dist1 == 0)
    {
      e1 = 1.0 * t1;
    } else
    {
      const double mh = 1.0 * ev->hequot[dist1];
      e1 = mh * t1;
    }
    if (dist2 == 0)
    {
      e2 = 1.0 * t2;
    } else
    {
      const double mh = 1.0 * ev->hequot[dist2];
      e2 = mh * t2;
    }
  }
  if (e1 < e2)
  {
    return -1;
  }
  if (e1 > e2)
  {
    return 1;
  }
  /* EVALIDENTITY, include/match.h:122-135 */
  q1 = (double) dist1 / (double) length1;
  q2 = (double) dist2 / (double) length2;
  id1 = 100.0 * (1.0 - q1);
  id2 = 100.0 * (1.0 - q2);
  if (id1 < id2)
  {
    return 1;
  }
  if (id1 > id2)
  {
    return -1;
  }
  return length1 > length2 ? -1 : 1;
}

/* the largest row + diagonal among the fronts h, h - 1, ..: the next lower
   front is looked at while the one before had an undefined entry
   (extendED.c:140-194) */
VSA_HD int64_t vsa_ed_maxextend(const vsa_ed_side *s, const VSA_ED_ROW *fronts,
                                uint32_t h)
{
  int64_t best = 0, i, k, lo, hi;
  int next = 1;

  for (i = (int64_t) h; next && i >= 0; i--)
  {
    next = 0;
    vsa_ed_range(s, i, &lo, &hi);
    for (k = lo; k <= hi; k++)
    {
      const VSA_ED_ROW v = fronts[vsa_ed_at(i, k)];
      if (v == VSA_ED_UNDEF)
      {
        next = 1;
      } else if ((int64_t) v + k > best)
      {
        best = (int64_t) v + k;
      }
    }
  }
  return best;
}

/* The best match of a seed of `length` symbols at pos1 / pos2 whose sides
   have the fronts lf / rf up to front hleft / hright.  self: both instances
   lie in one Multiseq (neither rcmode nor querycompare).  1: *best;
   0: nothing reaches leastlength. */
VSA_HD int vsa_ed_choose(const vsa_selrules *ev, const vsa_ed_side *ls,
                         const vsa_ed_side *rs, int self, uint64_t pos1,
                         uint64_t pos2, uint64_t length, uint64_t leastlength,
                         const VSA_ED_ROW *lf, uint32_t hleft,
                         const VSA_ED_ROW *rf, uint32_t hright,
                         vsa_ed_match *best)
{
  const int64_t remain =
      length >= leastlength ? 0 : (int64_t) (leastlength - length);
  const uint8_t *s1 = ls->s1, *s2 = ls->s2;
  int64_t maxdist = ls->maxdist, dist, li, lk, rk, llo, lhi, rlo, rhi;
  int found = 0;

  if (vsa_ed_maxextend(ls, lf, hleft) + vsa_ed_maxextend(rs, rf, hright) <
      remain)
  {
    return 0;
  }
  if ((int64_t) hleft + (int64_t) hright < maxdist)
  {
    maxdist = (int64_t) hleft + (int64_t) hright;
  }
  for (dist = 0; dist <= maxdist; dist++)
  {
    const int64_t top = dist < (int64_t) hleft ? dist : (int64_t) hleft;
    for (li = dist < (int64_t) hright ? 0 : dist - (int64_t) hright;
         li <= top; li++)
    {
      vsa_ed_range(ls, li, &llo, &lhi);
      vsa_ed_range(rs, dist - li, &rlo, &rhi);
      for (lk = llo; lk <= lhi; lk++)
      {
        const VSA_ED_ROW lv = lf[vsa_ed_at(li, lk)];
        if (lv == VSA_ED_UNDEF)
        {
          continue;
        }
        for (rk = rlo; rk <= rhi; rk++)
        {
          const VSA_ED_ROW rv = rf[vsa_ed_at(dist - li, rk)];
          int64_t exti, extj;
          uint64_t p1, p2, length1, length2;

          if (rv == VSA_ED_UNDEF)
          {
            continue;
          }
          exti = (int64_t) lv + (int64_t) rv;
          if (exti < remain)
          {
            continue;
          }
          extj = exti + lk + rk;
          if (extj < remain)
          {
            continue;
          }
          p1 = pos1 - (uint64_t) lv;
          p2 = (uint64_t) ((int64_t) pos2 - (int64_t) lv - lk);
          if (!self || p1 <= p2)
          {
            length1 = length + (uint64_t) exti;
            length2 = length + (uint64_t) extj;
          } else
          {
            const uint64_t tmp = p1;
            p1 = p2;
            p2 = tmp;
            length1 = length + (uint64_t) extj;
            length2 = length + (uint64_t) exti;
          }
          /* a separator at either end of either instance (:268-285) */
          if (s1[p1 + length1 - 1] == VSA_SEPARATOR)
          {
            length1--;
          }
          if (s1[p1] == VSA_SEPARATOR)
          {
            p1++;
            length1--;
          }
          if (s2[p2 + length2 - 1] == VSA_SEPARATOR)
          {
            length2--;
          }
          if (s2[p2] == VSA_SEPARATOR)
          {
            p2++;
            length2--;
          }
          if (self &&
              !vsa_ed_accept((uint64_t) dist, length1, p1, length2, p2))
          {
            continue;
          }
          if (!found ||
              vsa_ed_cmp(ev, best->dist, (uint64_t) dist,
                         best->length1 > best->length2 ? best->length1
                                                       : best->length2,
                         length1 > length2 ? length1 : length2) == 1)
          {
            found = 1;
            best->dist = (uint64_t) dist;
            best->pos1 = p1;
            best->pos2 = p2;
            best->length1 = length1;
            best->length2 = length2;
          }
        }
      }
    }
  }
  return found;
}

/* the record of a match: `seed` moved to it.  abs2: the seed's position2 in
   the query Multiseq (relpos2 moves by position2 - pos2, extendED.c:326-331) */
VSA_HD void vsa_ed_record(const vsa_match *seed, int self, uint64_t abs2,
                          const vsa_ed_match *e, vsa_match *out)
{
  out->length = VSA_EDIST_PACK(e->length1, e->length2, e->dist);
  out->dbstart = e->pos1;
  if (self)
  {
    out->queryseq = e->pos2;
    out->querystart = 0;
  } else
  {
    out->queryseq = seed->queryseq;
    out->querystart = seed->querystart - (abs2 - e->pos2);
  }
}

#endif
