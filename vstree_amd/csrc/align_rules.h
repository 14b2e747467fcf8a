/*
  The rules of vmatch -s, stated ONCE for the host (align_host.c) and for the
  kernels (align.hip): how the edit script of a match is made
  (Vmatch/echomatch.c:587-678 shownormalstringout; kurtz/galign.c:135-420 with
  kurtz/front.gen; include/alignment.h:43-46).  Plain C that both compilers
  read.  It builds on erate_rules.h, which states the greedy front of
  front.gen for the clustering by edit distance: vsa_er_symequal,
  vsa_er_sametext, vsa_er_stored, VSA_ER_NEG.

  The two substrings u (the left instance, in the index) and v (the right one)
  of a record: vsa_al_viewof says which lengths and which distance a record of
  each sink kind carries, vsa_al_fits whether it lies inside its texts, and
  vsa_al_vfirst where v begins.  For the pass over the reverse complement
  (palindromic) the record names a stretch of the reverse complement of a
  query sequence; v is then read BACKWARDS in the forward sequence, every
  symbol complemented (vsa_al_complement; a special symbol stays special) --
  the copy initseqinfoRC makes (echomatch.c:660-678).

  The script of a record with the stored distance D:
    D == 0   one identical run of the length (alignequalstrings);
    D < 0    (-h) back to front, a position with a != b or a special a is a
             mismatch (hammingalignment);
    D > 0    (-e) the greedy front: generation 0 slides from row 0 on diagonal
             0; generation g evaluates the diagonals -g .. g: the best of the
             three predecessors AND which one it was (vsa_al_direction: the
             replacement unless the insertion is strictly better, the deletion
             only if strictly better than both), the same-text shortcut of
             front.gen:120-123 (only where both substrings lie in one array),
             the slide, vsa_er_stored.  The direction is kept also where the
             entry becomes minus infinity.  The first g with
             front[vlen - ulen] == ulen is the real distance (vsa_al_ends); it
             may be smaller than D.  Then backtracefront from (ulen - 1,
             vlen - 1) on diagonal vlen - ulen, for g = distance .. 1: slide
             backwards BY COMPARING SYMBOLS while i >= 0 and j >= 0
             (vsa_al_slideback; it may pass the row the forward slide began
             at), an identical run if it moved, then the operation the
             direction of front(g, d) names (vsa_al_step).  A rest i >= 0 is
             one more identical run.
  The words of a script (16 bits, LAST OPERATION FIRST): a run length up to
  16383, VSA_AL_DELETION, VSA_AL_INSERTION, VSA_AL_MISMATCH.  A longer run is
  cut the way ADDIDENTICAL cuts it (vsa_al_identical; galign.c:78-89), which
  is kept literally although its pieces do not add up to the run.
  A script of distance d has at most vsa_al_maxwords words.

  What is not restated: the narrower fronts of generations above min(ulen,
  vlen) (front.gen:48-63).  A record whose stored distance is above one of
  its lengths is refused like one that does not fit its texts; no matcher
  reports such a match.
*/
#ifndef VSA_ALIGN_RULES_H
#define VSA_ALIGN_RULES_H
#include <stdint.h>
#include "vstree_amd.h"
#include "erate_rules.h"

/* include/alignment.h:43-46 */
#define VSA_AL_MAXRUN 16383u
#define VSA_AL_DELETION ((uint16_t) (1u << 14))
#define VSA_AL_INSERTION ((uint16_t) (1u << 15))
#define VSA_AL_MISMATCH ((uint16_t) (3u << 14))

/* where an entry of a front came from: two bits */
#define VSA_AL_REPLACEMENT 1
#define VSA_AL_INSERTED 2
#define VSA_AL_DELETED 3
/* the directions of one diagonal in one 64-bit word, generation g in bits
   2 g, 2 g + 1: generations 0 .. 31 */
#define VSA_AL_REGISTERGENS 32

VSA_CLHD uint64_t vsa_al_setdir(uint64_t reg, int64_t g, int dir)
{
  return reg | (uint64_t) dir << (2 * g);
}

VSA_CLHD int vsa_al_getdir(uint64_t reg, int64_t g)
{
  return (int) (reg >> (2 * g) & 3u);
}

/* ---- what a record names -------------------------------------------------- */

VSA_CLHD int vsa_al_covered(int kind)
{
  return (kind >= VSA_SINK_COMPLETE && kind <= VSA_SINK_APPROX_HAMMING) ||
         (kind >= VSA_SINK_QUERY_HAMMING && kind <= VSA_SINK_SELF_EDIST);
}

VSA_CLHD int vsa_al_isself(int kind)
{
  return kind == VSA_SINK_SELF || kind == VSA_SINK_SELF_HAMMING ||
         kind == VSA_SINK_SELF_EDIST;
}

typedef struct
{
  uint64_t length1, length2;
  uint64_t start2;  /* self: position2 in the index; else the place in the
                       query sequence the record refers to (for a palindromic
                       pass: in its reverse complement) */
  int64_t distance; /* as the reference stores it: > 0 edit operations, < 0
                       mismatches, 0 equal strings */
} vsa_al_view;

/* the view of record m of a list of `kind`; seqlength2: the length of its
   query sequence (unused for a self kind).  0, or -2 for a record no matcher
   delivers: an empty instance, unequal lengths without insertions, a distance
   the lengths cannot have or that is above one of them */
VSA_CLHD int vsa_al_viewof(int kind, const vsa_match *m, uint64_t seqlength2,
                           vsa_al_view *w)
{
  uint64_t ad, diff, shorter;

  w->start2 = vsa_al_isself(kind) ? m->queryseq : m->querystart;
  switch (kind)
  {
    case VSA_SINK_QUERY_EDIST:
    case VSA_SINK_SELF_EDIST:
      w->length1 = VSA_EDIST_LENGTH1(m->length);
      w->length2 = VSA_EDIST_LENGTH2(m->length);
      w->distance = (int64_t) VSA_EDIST_DISTANCE(m->length);
      break;
    case VSA_SINK_QUERY_HAMMING:
    case VSA_SINK_SELF_HAMMING:
      w->length1 = w->length2 = VSA_HAMMING_LENGTH(m->length);
      w->distance = -(int64_t) VSA_HAMMING_DISTANCE(m->length);
      break;
    case VSA_SINK_COMPLETE:
    case VSA_SINK_APPROX_EDIST:
    case VSA_SINK_APPROX_HAMMING:
      /* initcompletematchstruct, Vmengine/initcompl.c:7-21: the whole query */
      w->length1 = m->length;
      w->length2 = seqlength2;
      w->start2 = 0;
      if (m->querystart > VSA_EDIST_MAXDISTANCE && kind != VSA_SINK_COMPLETE)
      {
        return -2;
      }
      w->distance = kind == VSA_SINK_COMPLETE ? 0
                    : kind == VSA_SINK_APPROX_EDIST
                        ? (int64_t) m->querystart
                        : -(int64_t) m->querystart;
      break;
    default:
      w->length1 = w->length2 = m->length;
      w->distance = 0;
  }
  if (w->length1 == 0 || w->length2 == 0 || w->length1 >= (uint64_t) 1 << 48 ||
      w->length2 >= (uint64_t) 1 << 48)
  {
    return -2;
  }
  if (w->distance <= 0)
  {
    return w->length1 == w->length2 ? 0 : -2;
  }
  ad = (uint64_t) w->distance;
  diff = w->length1 > w->length2 ? w->length1 - w->length2
                                 : w->length2 - w->length1;
  shorter = w->length1 < w->length2 ? w->length1 : w->length2;
  return diff <= ad && ad <= shorter ? 0 : -2;
}

/* does the view lie inside its texts?  n1: the length of the index, room2:
   of the text the right instance lies in (the index again, or the query
   sequence) */
VSA_CLHD int vsa_al_fits(const vsa_al_view *w, uint64_t dbstart, uint64_t n1,
                         uint64_t room2)
{
  return dbstart <= n1 && w->length1 <= n1 - dbstart && w->start2 <= room2 &&
         w->length2 <= room2 - w->start2;
}

/* the offset of the first symbol of v from the start of its sequence; a
   palindromic v goes DOWN from there */
VSA_CLHD uint64_t vsa_al_vfirst(const vsa_al_view *w, uint64_t seqlength2,
                                int palindromic)
{
  return palindromic ? seqlength2 - 1 - w->start2 : w->start2;
}

/* makereversecomplement, kurtz-basic/readmulti.c:32-53 */
VSA_CLHD uint8_t vsa_al_complement(uint8_t c)
{
  return VSA_ER_ISSPECIAL(c) ? c : (uint8_t) (3u - c);
}

/* ---- the two substrings --------------------------------------------------- */

typedef struct
{
  const uint8_t *u, *v; /* symbol x of u is u[x]; of v it is v[x] or -- vrev
                           -- the complement of *(v - x) */
  uint64_t ulen, vlen;
  int vrev;
  /* both substrings lie in ONE array, at pu and pv (front.gen:120 compares
     pointers): the self kinds */
  int onearray;
  uint64_t pu, pv;
} vsa_al_pair;

VSA_CLHD uint8_t vsa_al_vsym(const vsa_al_pair *p, int64_t x)
{
  return p->vrev ? vsa_al_complement(*(p->v - x)) : p->v[x];
}

VSA_CLHD int vsa_al_sametext(const vsa_al_pair *p, int64_t k)
{
  return p->onearray && vsa_er_sametext(p->pu, p->ulen, p->pv, p->vlen, k);
}

/* ---- the front ------------------------------------------------------------ */

/* the best of the three predecessors of an entry -> *t, and which one it was
   (evalentryforward, front.gen:90-108) */
VSA_CLHD int vsa_al_direction(int64_t same, int64_t below, int64_t above,
                              int64_t *t)
{
  int dir = VSA_AL_REPLACEMENT;

  *t = same + 1;
  if (*t < below)
  {
    *t = below;
    dir = VSA_AL_INSERTED;
  }
  if (*t < above + 1)
  {
    *t = above + 1;
    dir = VSA_AL_DELETED;
  }
  return dir;
}

/* the row u[t ..) and v[t + k ..) agree up to, one symbol at a time */
VSA_CLHD int64_t vsa_al_slide(const vsa_al_pair *p, int64_t t, int64_t k)
{
  while (t < (int64_t) p->ulen && t + k < (int64_t) p->vlen &&
         vsa_er_symequal(p->u[t], vsa_al_vsym(p, t + k)))
  {
    t++;
  }
  return t;
}

/* what an entry needs besides its slide: 1 and the stored value in *value if
   there is nothing to slide along (front.gen:111-123) */
VSA_CLHD int vsa_al_noslide(const vsa_al_pair *p, int64_t t, int64_t k,
                            int64_t *value)
{
  if (t < 0 || t + k < 0)
  {
    *value = VSA_ER_NEG;
    return 1;
  }
  if (vsa_al_sametext(p, k))
  {
    *value = vsa_er_stored((int64_t) p->ulen - 1, k, p->ulen, p->vlen);
    return 1;
  }
  return 0;
}

/* front[k] of a generation >= 1 from the best predecessor t */
VSA_CLHD int64_t vsa_al_entry(const vsa_al_pair *p, int64_t t, int64_t k)
{
  int64_t value;

  if (vsa_al_noslide(p, t, k, &value))
  {
    return value;
  }
  return vsa_er_stored(vsa_al_slide(p, t, k), k, p->ulen, p->vlen);
}

/* the end test of a generation: the row of diagonal vlen - ulen */
VSA_CLHD int vsa_al_ends(int64_t row, uint64_t ulen)
{
  return row == (int64_t) ulen;
}

/* ---- the script ----------------------------------------------------------- */

/* 2 (d + 1) + min(ulen, vlen) / 16383 + 1: d operations, d + 1 runs, one more
   piece for every 16383 symbols of the runs (the reference reserves 2 (d + 1)
   and has no room for the pieces) */
VSA_CLHD uint64_t vsa_al_maxwords(uint64_t d, uint64_t ulen, uint64_t vlen)
{
  return 2 * (d + 1) + (ulen < vlen ? ulen : vlen) / VSA_AL_MAXRUN + 1;
}

/* ADDIDENTICAL: the pieces of a run of lenid >= 1 symbols to out (or, out ==
   NULL, nowhere) -> their number */
VSA_CLHD uint64_t vsa_al_identical(uint16_t *out, uint64_t lenid)
{
  uint64_t n = 0;

  for (;;)
  {
    if (out != NULL)
    {
      out[n] = (uint16_t) (lenid & VSA_AL_MAXRUN);
    }
    n++;
    if (lenid <= VSA_AL_MAXRUN)
    {
      return n;
    }
    lenid -= VSA_AL_MAXRUN;
  }
}

/* the symbols below (i, j) that agree, one at a time (backtracefront,
   galign.c:255-260) */
VSA_CLHD int64_t vsa_al_slideback(const vsa_al_pair *p, int64_t i, int64_t j)
{
  int64_t run = 0;

  while (i - run >= 0 && j - run >= 0 &&
         vsa_er_symequal(p->u[i - run], vsa_al_vsym(p, j - run)))
  {
    run++;
  }
  return run;
}

/* the operation of a direction, applied to the place (i, j) on diagonal d;
   the order of the tests is the reference's (galign.c:266-291) */
VSA_CLHD uint16_t vsa_al_step(int dir, int64_t *i, int64_t *j, int64_t *d)
{
  if (dir == VSA_AL_REPLACEMENT)
  {
    (*i)--;
    (*j)--;
    return VSA_AL_MISMATCH;
  }
  if (dir == VSA_AL_DELETED)
  {
    (*i)--;
    (*d)++;
    return VSA_AL_DELETION;
  }
  (*j)--;
  (*d)--;
  return VSA_AL_INSERTION;
}

/* hammingalignment's test of one column */
VSA_CLHD int vsa_al_mismatch(uint8_t a, uint8_t b)
{
  return a != b || VSA_ER_ISSPECIAL(a);
}

/* the Hamming script of u and v (ulen symbols each), back to front, to out
   (or nowhere) -> its words.  The equal-string script is
   vsa_al_identical(out, ulen). */
VSA_CLHD uint64_t vsa_al_hamming(const vsa_al_pair *p, uint16_t *out)
{
  uint64_t n = 0, lenid = 0;
  int64_t i;

  for (i = (int64_t) p->ulen - 1; i >= 0; i--)
  {
    if (vsa_al_mismatch(p->u[i], vsa_al_vsym(p, i)))
    {
      if (lenid > 0)
      {
        n += vsa_al_identical(out != NULL ? out + n : NULL, lenid);
        lenid = 0;
      }
      if (out != NULL)
      {
        out[n] = VSA_AL_MISMATCH;
      }
      n++;
    } else
    {
      lenid++;
    }
  }
  if (lenid > 0)
  {
    n += vsa_al_identical(out != NULL ? out + n : NULL, lenid);
  }
  return n;
}

#endif
