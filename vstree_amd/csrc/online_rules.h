/*
  The rules of the scan without an index (vmatch -online -complete), stated
  ONCE for the host (online_host.c) and for the kernels (online.hip): what
  findexactcompletematchesonline (Vmengine/exactcompl.c:277-325),
  hammingcompletematchesonline (hamcompl.c:9-56) and
  findedistcompletematchesonline (edistcompl.c:14-172, 261-384, 458-513) with
  edistprocessstartpos (approxcompl.c:14-65) report, where that differs from
  the indexed search.  Plain C that both compilers read.

    thresholds  K, or m K / 100 for Kp (initcompl.c:52-56).  With -e a
                threshold of 0 still takes the scan of the columns; nothing
                in the online code refuses a threshold >= m.
    equality    exact: a window matches if no TEXT symbol of it is special
                and all symbols are equal (exactcompl.c:309).
                -h: bytes as they are, so a wildcard equals a wildcard; a
                window that holds a separator is no match (hamcompl.c:28-40).
                -e, m <= 64: the Eqsrev masks of kurtz-basic/getEqs.gen:27-49,
                in which a wildcard of the pattern sets no bit: a wildcard
                equals nothing.  -e, m > 64: edistukkonencutoff compares
                bytes (edistcompl.c:123): a wildcard equals a wildcard.  The
                word boundary is 64 here (ISLARGEPATTERN8); the indexed
                verification has it at 32.
    start       every position whose bottom score is <= the threshold, the
                text scanned from right to left with the reversed pattern, a
                separator resets the column (edistcompl.c:285-307).
    maxlength   min(m + k, totallength - start) (SETMAXLENGTH,
                edistcompl.c:14-19), not the width of a region.
    longest     the best-distance, then longest prefix (longestmatch.c): there
                a wildcard equals nothing for every m (:52, and getEqs.gen for
                the masks), and the distance is reported as it comes, above K
                too (approxcompl.c:52-59 checks it in the debug build only).
    remred      CHECKMATCHPOSITION, edistcompl.c:33-80: vsa_online_remred_*.
*/
#ifndef VSA_ONLINE_RULES_H
#define VSA_ONLINE_RULES_H
#include <stdint.h>
#include "vstree_amd.h"

#ifndef VSA_HD
#ifdef __HIPCC__
#define VSA_HD __host__ __device__ static inline
#else
#define VSA_HD static inline
#endif
#endif

#define VSA_ONLINE_EXACT 0
#define VSA_ONLINE_EDIST 1
#define VSA_ONLINE_HAMMING 2

/* initcompl.c:52-56, :78 */
VSA_HD uint64_t vsa_online_threshold(uint64_t m, uint64_t distvalue,
                                     int percent)
{
  return percent ? (m * distvalue) / 100 : distvalue;
}

/* ISLARGEPATTERN8, edistcompl.c:467: the scan of the columns compares bytes */
VSA_HD int vsa_online_rawequal(uint64_t m)
{
  return m > 64;
}

/* does pattern symbol p set the bit of text symbol c in the scan for start
   positions? */
VSA_HD int vsa_online_scanequal(uint8_t p, uint8_t c, int rawequal)
{
  return p == c && (rawequal || p != (uint8_t) VSA_WILDCARD);
}

/* ... and in longestmatch.c */
VSA_HD int vsa_online_longestequal(uint8_t p, uint8_t c)
{
  return p == c && p != (uint8_t) VSA_WILDCARD;
}

VSA_HD int vsa_online_isstart(uint64_t score, uint64_t k)
{
  return score <= k;
}

/* Symbols to the right of a piece of the text that a column started cold
   must have seen before its scores count.  A cold column holds D_cold >=
   D_true everywhere, and the two are equal wherever the best alignment ends
   before the cold start; an alignment of at most k errors uses at most m + k
   text symbols.  So behind m + k symbols "score <= k" is the reference's
   test and every score <= k is the reference's score.
   A separator resets both columns and only makes them equal sooner. */
VSA_HD uint64_t vsa_online_warmup(uint64_t m, uint64_t k)
{
  return m + k;
}

/* SETMAXLENGTH */
VSA_HD uint64_t vsa_online_maxlength(uint64_t m, uint64_t k,
                                     uint64_t totallength, uint64_t start)
{
  const uint64_t rest = totallength - start;
  return rest > m + k ? m + k : rest;
}

/* -complete remred.  The state travels along the start positions of ONE
   pattern in the order they are found (descending).  A hit directly in front
   of the stored position replaces it only with a smaller score; a hit there
   that does not improve changes nothing, relpos stays, and so the next hit
   is not adjacent any more: the stored one is flushed and the hit that did
   not improve is never reported.  A separator does not touch the state. */
typedef struct
{
  uint64_t relpos, distance;
  int found;
} vsa_online_remred;

VSA_HD void vsa_online_remred_init(vsa_online_remred *s)
{
  s->relpos = s->distance = 0;
  s->found = 0;
}

/* a hit at `pos` with `score`; 1: *flush is a start position to report */
VSA_HD int vsa_online_remred_step(vsa_online_remred *s, uint64_t pos,
                                  uint64_t score, uint64_t *flush)
{
  if (s->found)
  {
    if (s->relpos == pos + 1)
    {
      if (score < s->distance)
      {
        s->relpos = pos;
        s->distance = score;
      }
      return 0;
    }
    *flush = s->relpos;
    s->relpos = pos;
    s->distance = score;
    return 1;
  }
  s->relpos = pos;
  s->distance = score;
  s->found = 1;
  return 0;
}

/* the end of the text */
VSA_HD int vsa_online_remred_end(const vsa_online_remred *s, uint64_t *flush)
{
  *flush = s->relpos;
  return s->found;
}

/* Eight symbols of a window at a time, the first one in the lowest byte,
   `count` (1 .. 8) of them valid.  -> the number of unequal bytes; *barred
   != 0: a symbol of the text that bars the window, i.e. a separator (-h) or
   any special symbol (exact). */
VSA_HD uint32_t vsa_online_word(uint64_t tw, uint64_t pw, uint32_t count,
                                int mode, int *barred)
{
  const uint64_t H = 0x8080808080808080ull, L = 0x7F7F7F7F7F7F7F7Full,
                 valid = count >= 8 ? ~0ull : ((1ull << (8 * count)) - 1),
                 x = (tw ^ pw) & valid,
                 ne = (((x & L) + L) | x) & H,
                 /* bytes that are 0 here are 255 (or 254, 255) in the text */
                 z = ~(mode == VSA_ONLINE_EXACT
                           ? (tw | 0x0101010101010101ull)
                           : tw),
                 nz = (((z & L) + L) | z) & H;

  *barred = ((~nz & H) & valid) != 0;
  return (uint32_t) __builtin_popcountll(ne);
}

#endif
