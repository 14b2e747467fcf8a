/*
  The rules of the Hamming extension of exact seeds (vmatch -l L -h K outside
  -complete), stated ONCE for the host (extend_host.c) and for the kernels
  (extend.hip): the seed length (Vmatch/matchlenparm.c:11-22), the two look
  tables with their border branches (hammingextend, kurtz/extendHD.c:56-264)
  and the choice among the extensions (:265-358 with cmpmatches,
  include/extcmp.c).  Plain C that both compilers read; the double operations
  are one table read, one division, one subtraction and one multiplication, in
  the reference's order, so host and device agree bit for bit.

  A Multiseq is seen through a VIEW: the stretch of symbols a seed can be
  extended in, and whether the stretch begins / ends the Multiseq.  The text
  of the index is one stretch with its separators as symbols.  A query
  sequence of a batch is a stretch of its own: whatever lies around it in
  memory (nothing in a dense batch of reads), the reference's Multiseq has a
  separator there, which the view supplies, unless the sequence is the first /
  last one, where the Multiseq ends.

  A side of a seed is scanned as a sequence of EVENTS at offsets t = 0, 1, ..
  from the second symbol beside the seed (the symbol directly beside a maximal
  seed is never compared): a separator, a mismatch (a wildcard never matches),
  or the border of the Multiseq.  However the symbols are read -- byte by
  byte, in words of 8, by a wavefront in steps of 1024 -- the table is what
  the events make of it.
*/
#ifndef VSA_EXTEND_RULES_H
#define VSA_EXTEND_RULES_H
#include <stdint.h>
#include "vstree_amd.h"
#include "select_rules.h"

/* Matchparam.seedlength, Vmatch/matchlenparm.c:11-22 */
VSA_HD uint64_t vsa_ext_seedlength(uint64_t leastlength, uint64_t maxdist,
                                   uint64_t seedlength)
{
  const uint64_t least = leastlength / (maxdist + 1);

  return seedlength > least ? seedlength : least;
}

typedef struct
{
  const uint8_t *p; /* the symbols of the stretch, p[0 .. len)          */
  uint64_t len;
  int atstart;      /* the stretch begins at position 0 of the Multiseq */
  int atend;        /* ... ends at its last position                    */
} vsa_ext_view;

/* the symbol at place i of the stretch, a separator around it */
VSA_HD uint8_t vsa_ext_sym(const vsa_ext_view *v, int64_t i)
{
  return (i < 0 || (uint64_t) i >= v->len) ? (uint8_t) VSA_SEPARATOR
                                           : v->p[i];
}

/* ---- one look table in the making ------------------------------------- */

#ifndef VSA_EXT_LOOK
#define VSA_EXT_LOOK uint64_t /* an entry of a look table */
#endif

typedef struct
{
  VSA_EXT_LOOK *look; /* entry h at look[h * stride]; NULL: not written  */
  uint64_t stride;
  uint64_t seedlength;
  uint64_t prev, last; /* look[h - 1], and the entry written last       */
  uint32_t h, maxdist;
  int left;            /* the left scan, with its stop rule              */
} vsa_ext_scan;

VSA_HD void vsa_ext_put(vsa_ext_scan *s, uint64_t value)
{
  s->last = value;
  if (s->look != NULL)
  {
    s->look[(uint64_t) s->h * s->stride] = (VSA_EXT_LOOK) value;
  }
}

VSA_HD void vsa_ext_begin(vsa_ext_scan *s, VSA_EXT_LOOK *look,
                          uint64_t stride, uint32_t maxdist,
                          uint64_t seedlength, int left)
{
  s->look = look;
  s->stride = stride;
  s->seedlength = seedlength;
  s->maxdist = maxdist;
  s->left = left;
  s->h = 0;
  vsa_ext_put(s, 0);
  s->prev = 0;
  s->h = 1;
}

/* the three events; 1: the scan is over */
VSA_HD int vsa_ext_separator(vsa_ext_scan *s, uint64_t t)
{
  vsa_ext_put(s, t + 1);
  return 1;
}

VSA_HD int vsa_ext_mismatch(vsa_ext_scan *s, uint64_t t)
{
  vsa_ext_put(s, t + 1);
  /* extendHD.c:89: the left scan stops behind an exact stretch longer than
     the seed length, the right scan (:149) does not */
  if (s->h == s->maxdist || (s->left && t + 1 - s->prev > s->seedlength))
  {
    return 1;
  }
  s->prev = t + 1;
  s->h++;
  return 0;
}

VSA_HD int vsa_ext_border(vsa_ext_scan *s, uint64_t t)
{
  vsa_ext_put(s, t + 2);
  return 1;
}

/* the number of mismatches the side offers, extendHD.c:105-113,162-163 */
VSA_HD uint32_t vsa_ext_end(const vsa_ext_scan *s)
{
  return (s->left && s->last - s->prev > s->seedlength) ? s->h - 1 : s->h;
}

/* ---- the border branches, extendHD.c:198-264 --------------------------- */

typedef struct
{
  const uint8_t *p1, *p2; /* the symbols at t = 0                         */
  uint64_t nsym;          /* symbols to look at: t = 0 .. nsym - 1        */
  int endsep;             /* behind them: 1 a separator the view supplies
                             at t = nsym, 0 the border at t = nsym - 1    */
} vsa_ext_plan;

#define VSA_EXT_FIXED 0 /* the table is complete: *h entries beyond [0]  */
#define VSA_EXT_SCAN 1  /* *plan says what to scan                        */

/* a seed of `length` symbols at pos1 of view 1 and pos2 of view 2, which it
   fits (the caller has checked).  Writes look[0] = 0 and, where a branch
   grants one symbol with one mismatch unseen, look[1] = 1. */
VSA_HD int vsa_ext_prepare(vsa_ext_scan *s, const vsa_ext_view *v1,
                           uint64_t pos1, const vsa_ext_view *v2,
                           uint64_t pos2, uint64_t length, vsa_ext_plan *plan,
                           uint32_t *h)
{
  const uint64_t none = ~(uint64_t) 0;
  uint64_t border = none, vsep = none;

  if (s->left)
  {
    const int in1 = !v1->atstart || pos1 > 1,
              in2 = !v2->atstart || pos2 > 1;
    if ((v1->atstart && pos1 == 0) || (v2->atstart && pos2 == 0) ||
        vsa_ext_sym(v1, (int64_t) pos1 - 1) == VSA_SEPARATOR ||
        vsa_ext_sym(v2, (int64_t) pos2 - 1) == VSA_SEPARATOR)
    {
      *h = 0;
      return VSA_EXT_FIXED;
    }
    if (!(in1 && in2))
    {
      vsa_ext_put(s, 1); /* extendHD.c:225-227 */
      *h = 1;
      return VSA_EXT_FIXED;
    }
    /* t = 0 is place pos - 2: the border at place 0, the separator of the
       view at place -1 */
    if (v1->atstart)
    {
      border = pos1 - 2;
    } else
    {
      vsep = pos1 - 1;
    }
    if (v2->atstart)
    {
      border = pos2 - 2 < border ? pos2 - 2 : border;
    } else
    {
      vsep = pos2 - 1 < vsep ? pos2 - 1 : vsep;
    }
    plan->p1 = v1->p + pos1 - 2;
    plan->p2 = v2->p + pos2 - 2;
  } else
  {
    const uint64_t e1 = pos1 + length, e2 = pos2 + length;
    const int in1 = !v1->atend || e1 + 1 < v1->len,
              in2 = !v2->atend || e2 + 1 < v2->len;
    if ((v1->atend && e1 >= v1->len) || (v2->atend && e2 >= v2->len) ||
        vsa_ext_sym(v1, (int64_t) e1) == VSA_SEPARATOR ||
        vsa_ext_sym(v2, (int64_t) e2) == VSA_SEPARATOR)
    {
      *h = 0;
      return VSA_EXT_FIXED;
    }
    if (!(in1 && in2))
    {
      vsa_ext_put(s, 1); /* extendHD.c:260-262 */
      *h = 1;
      return VSA_EXT_FIXED;
    }
    /* t = 0 is place e + 1: the border at place len - 1, the separator of
       the view at place len */
    if (v1->atend)
    {
      border = v1->len - e1 - 2;
    } else
    {
      vsep = v1->len - e1 - 1;
    }
    if (v2->atend)
    {
      border = v2->len - e2 - 2 < border ? v2->len - e2 - 2 : border;
    } else
    {
      vsep = v2->len - e2 - 1 < vsep ? v2->len - e2 - 1 : vsep;
    }
    plan->p1 = v1->p + e1 + 1;
    plan->p2 = v2->p + e2 + 1;
  }
  /* at the same t the separator is seen first (extendHD.c:79,98) */
  if (vsep <= border)
  {
    plan->nsym = vsep;
    plan->endsep = 1;
  } else
  {
    plan->nsym = border + 1;
    plan->endsep = 0;
  }
  return VSA_EXT_SCAN;
}

/* the event behind the last symbol of the plan */
VSA_HD int vsa_ext_finish(vsa_ext_scan *s, const vsa_ext_plan *plan)
{
  return plan->endsep ? vsa_ext_separator(s, plan->nsym)
                      : vsa_ext_border(s, plan->nsym - 1);
}

/* ---- eight symbols at a time -------------------------------------------- */

#define VSA_EXT_HI 0x8080808080808080ull
#define VSA_EXT_LO 0x0101010101010101ull

/* the top bit of every byte of x that is not 0 */
VSA_HD uint64_t vsa_ext_nonzero(uint64_t x)
{
  return (((x & ~VSA_EXT_HI) + ~VSA_EXT_HI) | x) & VSA_EXT_HI;
}

/* a and b hold eight symbols each, symbol k of the word in bits 8k .. 8k+7.
   Bit k of the result: the symbols k differ or one of them is special (a
   mismatch or a separator); bit k of *sep: one of them is a separator. */
VSA_HD uint32_t vsa_ext_marks8(uint64_t a, uint64_t b, uint32_t *sep)
{
  /* a byte >= 254 (wildcard, separator) has all bits but the lowest set */
  const uint64_t special = ~vsa_ext_nonzero(~(a | VSA_EXT_LO)) |
                           ~vsa_ext_nonzero(~(b | VSA_EXT_LO));
  const uint64_t seps = (~vsa_ext_nonzero(~a) | ~vsa_ext_nonzero(~b)) &
                        VSA_EXT_HI;
  const uint64_t marks = (vsa_ext_nonzero(a ^ b) | special) & VSA_EXT_HI;
  /* the top bits of the eight bytes as one byte: bit 8k + 7 times 2^(7j)
     lands on bit 56 + k for j = 7 - k only, and no two products meet */
  const uint64_t gather = 0x0002040810204081ull;

  *sep = (uint32_t) ((seps * gather) >> 56);
  return (uint32_t) ((marks * gather) >> 56);
}

/* eight symbols at t0 .. t0 + 7 of a side as one word in the order of t:
   rightwards they lie at p + t0 upwards, leftwards at p - t0 downwards.  Of
   the eight only `valid` are in memory that may be read (the others read 0). */
VSA_HD uint64_t vsa_ext_word(const uint8_t *p, int left, uint64_t t0,
                             uint64_t valid)
{
  uint64_t w = 0;
  uint32_t k;

  for (k = 0; k < 8 && k < valid; k++)
  {
    const uint8_t c = left ? *(p - t0 - k) : *(p + t0 + k);
    w |= (uint64_t) c << (8 * k);
  }
  return w;
}

/* the events of the marks of one word whose first symbol is at t0, up to the
   last symbol of the plan; 1: the scan is over */
VSA_HD int vsa_ext_events(vsa_ext_scan *s, const vsa_ext_plan *plan,
                          uint64_t t0, uint32_t marks, uint32_t sep)
{
  uint32_t k;

  for (k = 0; marks >> k != 0; k++)
  {
    if (marks >> k & 1u)
    {
      if (t0 + k >= plan->nsym)
      {
        return 0;
      }
      if ((sep >> k & 1u) ? vsa_ext_separator(s, t0 + k)
                          : vsa_ext_mismatch(s, t0 + k))
      {
        return 1;
      }
    }
  }
  return 0;
}

/* ---- the choice, extendHD.c:265-358 --------------------------------------- */

/* cmpmatches (include/extcmp.c): E-value, then identity, then length; a tie
   answers 1, so the later candidate wins */
VSA_HD int vsa_ext_cmp(const vsa_selrules *ev, uint64_t dist1, uint64_t dist2,
                       uint64_t length1, uint64_t length2)
{
  double e1 = 0.0, e2 = 0.0, q1, q2, id1, id2;

  if (!ev->noevalue)
  {
    /* incgetEvalue(evalues, 1.0, -dist, length) */
    e1 = 1.0 * vsa_sel_lookup(ev, (int64_t) dist1, length1);
    e2 = 1.0 * vsa_sel_lookup(ev, (int64_t) dist2, length2);
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

/* The best extension of a seed of `length` symbols whose sides offer hleft /
   hright mismatches with the tables lookleft / lookright (entry h at
   [h * stride]).  1: *shift symbols to the left, *outlength symbols in all,
   *dist mismatches; 0: the seed cannot reach leastlength. */
VSA_HD int vsa_ext_choose(const vsa_selrules *ev, uint64_t length,
                          uint64_t leastlength, uint64_t maxdist,
                          const VSA_EXT_LOOK *lookleft, uint32_t hleft,
                          const VSA_EXT_LOOK *lookright, uint32_t hright,
                          uint64_t stride, uint64_t *shift,
                          uint64_t *outlength, uint64_t *dist)
{
  const uint64_t remain = length >= leastlength ? 0 : leastlength - length;
  uint64_t d, li;
  int found = 0;

  if ((uint64_t) lookleft[hleft * stride] +
          (uint64_t) lookright[hright * stride] < remain)
  {
    return 0;
  }
  if ((uint64_t) hleft + hright < maxdist)
  {
    maxdist = (uint64_t) hleft + hright; /* extendHD.c:283-286 */
  }
  for (d = 0; d <= maxdist; d++)
  {
    const uint64_t top = d < hleft ? d : hleft;
    for (li = d < hright ? 0 : d - hright; li <= top; li++)
    {
      const uint64_t ll = lookleft[li * stride];
      const uint64_t ext = ll + (uint64_t) lookright[(d - li) * stride];
      if (ext >= remain &&
          (!found ||
           vsa_ext_cmp(ev, *dist, d, *outlength, length + ext) == 1))
      {
        found = 1;
        *dist = d;
        *outlength = length + ext;
        *shift = ll;
      }
    }
  }
  return found;
}

#endif
