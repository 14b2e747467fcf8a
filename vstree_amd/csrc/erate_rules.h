/*
  The rules of vmatch -pp matchcluster erate E, stated ONCE for the host
  (matchcluster_host.c) and for the kernels (matchcluster_erate.inc): which
  pairs of matches i < j are linked, and with which value
  (Vmatch/cluedist.c:42-198, kurtz/frontSEP.c:341-446, kurtz/front.gen:48-213).
  Both instances of a match have its one length.  Plain C that both compilers
  read; the bound is one conversion, one multiplication and one division of
  doubles, so host and device agree bit for bit.

  The pair (i, j), i < j:
    minlen  = min(len_i, len_j), maxdist = vsa_er_maxdist(minlen, E);
    the instance pairs (1,1), (1,2), (2,1), (2,2) -- instance of i first --
    are tried in this order (vsa_er_first, vsa_er_second); the FIRST one whose
    answer is >= 0 stores the edge (i, j, vsa_er_value(minlen, answer)).
  The answer of an instance pair u = text[pu, pu + ulen), v = text[pv,
  pv + vlen):
    -1 if the lengths differ by more than maxdist (vsa_er_lengthfails);
    0 if pu == pv and ulen == vlen, whatever the text holds
    (vsa_er_sameinstance);
    else the greedy front of the unit edit distance, rounds 0 .. maxdist, all
    diagonals -d .. d in round d (maxdist <= minlen: the reference's narrower
    fronts for d > minlen never occur):
      round 0   front[0] = vsa_er_slide from row 0;
      round d   t = max(prev[k] + 1, prev[k - 1], prev[k + 1] + 1);
                vsa_er_entry makes the value of the diagonal of it;
      the answer is the first d with front[vlen - ulen] == ulen, or -1 after
      maxdist rounds.  With maxdist == 0 that is round 0 alone: 0 iff both
      substrings are equal symbol for symbol and hold no special symbol.
  A special symbol (wildcard, separator) equals nothing, not even itself
  (vsa_er_symequal).

  One thing the reference does is no textbook front and is kept, because
  what it prints depends on it (front.gen:120-123): in a round d >= 1, a
  diagonal on which both substrings are THE SAME TEXT (pu + t == pv + t + k)
  is not slid along; its row becomes ulen - 1, even where that is a step
  back or where a special symbol lies ahead.  Matches that overlap in the
  text meet this all the time.  Without a separator inside an instance the
  bounds of COMPARESYMBOLS never move; vsa_matchcluster_add refuses records
  that hold one.
*/
#ifndef VSA_ERATE_RULES_H
#define VSA_ERATE_RULES_H
#include <stdint.h>
#include "vstree_amd.h"
#include "select_rules.h"
#include "cluster_rules.h"

/* what becomes of a pair i < j: classes of the compaction */
#define VSA_ER_SURVIVOR 0 /* passed the length test                         */
#define VSA_ER_TOOFAR 1   /* ... but its bound is above VSA_ERATE_MAXDIST   */
#define VSA_ER_LENGTH 2   /* failed the length test                         */
#define VSA_ER_CLASSES 3

/* "no row": below every row, and still below 0 after maxdist increments */
#define VSA_ER_NEG (-((int64_t) 1 << 40))

VSA_CLHD uint64_t vsa_er_maxdist(uint64_t minlen, uint32_t errorrate)
{
  const double scaled = (double) minlen * (double) errorrate;
  return (uint64_t) (scaled / 100.0);
}

/* the same answer for all four instance pairs: both instances of a match
   have one length */
VSA_CLHD int vsa_er_lengthfails(uint64_t len_i, uint64_t len_j,
                                uint64_t maxdist)
{
  return (len_i > len_j ? len_i - len_j : len_j - len_i) > maxdist;
}

VSA_CLHD int vsa_er_sameinstance(uint64_t pu, uint64_t ulen, uint64_t pv,
                                 uint64_t vlen)
{
  return ulen == vlen && pu == pv;
}

#define VSA_ER_ISSPECIAL(c) ((uint8_t) (c) >= (uint8_t) VSA_WILDCARD)

VSA_CLHD int vsa_er_symequal(uint8_t a, uint8_t b)
{
  return a == b && !VSA_ER_ISSPECIAL(a);
}

/* instance pair c = 0 .. 3 of the cascade: 1 -> position2 */
VSA_CLHD int vsa_er_first(int c)
{
  return c >> 1;
}

VSA_CLHD int vsa_er_second(int c)
{
  return c & 1;
}

VSA_CLHD uint64_t vsa_er_value(uint64_t minlen, uint64_t edist)
{
  return minlen << 32 | edist;
}

/* the maximum of the three predecessors */
VSA_CLHD int64_t vsa_er_best(int64_t same, int64_t below, int64_t above)
{
  int64_t t = same + 1;
  if (t < below)
  {
    t = below;
  }
  if (t < above + 1)
  {
    t = above + 1;
  }
  return t;
}

/* the diagonal k is the same text in both substrings (front.gen:120) */
VSA_CLHD int vsa_er_sametext(uint64_t pu, uint64_t ulen, uint64_t pv,
                             uint64_t vlen, int64_t k)
{
  return ulen != 0 && vlen != 0 && (int64_t) pu == (int64_t) pv + k;
}

/* the row after the slide (or the step of vsa_er_sametext) -> what the
   front stores (front.gen:135-141) */
VSA_CLHD int64_t vsa_er_stored(int64_t t, int64_t k, uint64_t ulen,
                               uint64_t vlen)
{
  return t > (int64_t) ulen || t + k > (int64_t) vlen ? VSA_ER_NEG : t;
}

/* the row that u[t ..) and v[t + k ..) agree up to, one symbol at a time */
VSA_CLHD int64_t vsa_er_slide(const uint8_t *text, uint64_t pu, uint64_t ulen,
                              uint64_t pv, uint64_t vlen, int64_t t, int64_t k)
{
  while (t < (int64_t) ulen && t + k < (int64_t) vlen &&
         vsa_er_symequal(text[pu + (uint64_t) t],
                         text[pv + (uint64_t) (t + k)]))
  {
    t++;
  }
  return t;
}

/* front[k] of a round d >= 1 from vsa_er_best of the round before */
VSA_CLHD int64_t vsa_er_entry(const uint8_t *text, uint64_t pu, uint64_t ulen,
                              uint64_t pv, uint64_t vlen, int64_t t, int64_t k)
{
  if (t < 0 || t + k < 0)
  {
    return VSA_ER_NEG;
  }
  t = vsa_er_sametext(pu, ulen, pv, vlen, k)
          ? (int64_t) ulen - 1
          : vsa_er_slide(text, pu, ulen, pv, vlen, t, k);
  return vsa_er_stored(t, k, ulen, vlen);
}

/* a record of the list before a look at the text: 0, VSA_NOT_COVERED for a
   length of 2^32 or more, -2 for one that leaves the text */
VSA_CLHD int vsa_er_checkplace(uint64_t textlength, uint64_t length,
                               uint64_t position1, uint64_t position2)
{
  if (length >= (uint64_t) 1 << 32)
  {
    return VSA_NOT_COVERED;
  }
  if (position1 > textlength || length > textlength - position1 ||
      position2 > textlength || length > textlength - position2)
  {
    return -2;
  }
  return 0;
}

/* ... and -2 for one that holds a separator (the kernel asks the same of
   eight symbols per load, er_hasseparator) */
VSA_CLHD int vsa_er_checkrecord(const uint8_t *text, uint64_t textlength,
                                uint64_t length, uint64_t position1,
                                uint64_t position2)
{
  const int rc = vsa_er_checkplace(textlength, length, position1, position2);
  uint64_t x;

  if (rc != 0)
  {
    return rc;
  }
  for (x = 0; x < length; x++)
  {
    if (text[position1 + x] == VSA_SEPARATOR ||
        text[position2 + x] == VSA_SEPARATOR)
    {
      return -2;
    }
  }
  return 0;
}

/* ---- what matchcluster.hip needs of matchcluster_host.c ------------------ */
#ifdef __cplusplus
extern "C" {
#endif

/* 0, or the message and the code of vsa_eratecluster_open; on success
   *rules is the view of a match of a self list */
int vsa_er_checklayout(const vsa_sinkparams *layout, uint32_t errorrate,
                       uint64_t textlength, const char *who,
                       vsa_selrules *rules);

#ifdef __cplusplus
}
#endif

#endif
