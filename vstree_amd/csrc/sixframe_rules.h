/*
  The rules of the six-frame translation, stated ONCE for the host
  (translate_host.c) and for the kernels (translate.hip): what vmatch
  -dnavsprot transnum -q Q PROTIDX makes of its DNA queries before the query
  engine sees them, and how it carries a match back to the DNA
  (kurtz/sixframe.c:70-143,232-264, kurtz/codon.c:292-550,605-870,939-999,
  Vmatch/procmatch.c:450-460, Vmatch/procfinal.c:262-289).  Plain C that both
  compilers read.

  Bases are numbered in the order of the NCBI genetic code tables, T 0, C 1,
  A 2, G 3; a character is a SET of bases, one bit per base (bit = 1 << base).
  A codon of three plain bases has the code 16 b0 + 4 b1 + b2.
*/
#ifndef VSA_SIXFRAME_RULES_H
#define VSA_SIXFRAME_RULES_H
#include <stdint.h>
#include "vstree_amd.h"

#ifdef __HIPCC__
#define VSA_SFHD __host__ __device__ static inline
#else
#define VSA_SFHD static inline
#endif

#define VSA_SF_T 1u
#define VSA_SF_C 2u
#define VSA_SF_A 4u
#define VSA_SF_G 8u
#define VSA_SF_FRAMES 6u
/* complement of every base of a codon code: T <-> A, C <-> G */
#define VSA_SF_COMPLEMENT 0x2Au

/* The base set of a DNA character, 0 for a character the translation does
   not know (codon.c:708-870: "illegal char").  Either case; U is T.  W stands
   for {A, C} here, not for {A, T}: that is the reference's table
   (codon.c:381,413), reproduced. */
VSA_SFHD uint32_t vsa_sf_class(uint8_t ch)
{
  switch (ch | 0x20u) /* only letters become lower-case letters */
  {
    case 'a': return VSA_SF_A;
    case 'c': return VSA_SF_C;
    case 'g': return VSA_SF_G;
    case 't':
    case 'u': return VSA_SF_T;
    case 'n': return VSA_SF_A | VSA_SF_C | VSA_SF_G | VSA_SF_T;
    case 's': return VSA_SF_C | VSA_SF_G;
    case 'y': return VSA_SF_C | VSA_SF_T;
    case 'w': return VSA_SF_A | VSA_SF_C;
    case 'r': return VSA_SF_A | VSA_SF_G;
    case 'k': return VSA_SF_G | VSA_SF_T;
    case 'v': return VSA_SF_A | VSA_SF_C | VSA_SF_G;
    case 'b': return VSA_SF_C | VSA_SF_G | VSA_SF_T;
    case 'd': return VSA_SF_A | VSA_SF_G | VSA_SF_T;
    case 'h': return VSA_SF_A | VSA_SF_C | VSA_SF_T;
    case 'm': return VSA_SF_A | VSA_SF_C;
    default: return 0;
  }
}

VSA_SFHD int vsa_sf_isplain(uint32_t cls)
{
  return cls != 0 && (cls & (cls - 1)) == 0;
}

/* the smallest base of a set in the order T < C < A < G */
VSA_SFHD uint32_t vsa_sf_smallest(uint32_t cls)
{
  return (cls & VSA_SF_T) ? 0u : (cls & VSA_SF_C) ? 1u
                                : (cls & VSA_SF_A) ? 2u : 3u;
}

/* A sequence shorter than three characters has no codon in any frame: its
   characters are never looked at.  In a longer one every character lies in a
   codon of some frame. */
VSA_SFHD int vsa_sf_illegal(uint64_t len, uint32_t cls)
{
  return len >= 3 && cls == 0;
}

/* the base of codon position 0 or 1, and of position 2 where it is plain: a
   plain base is complemented in the reverse frames, the smallest base of a
   wildcard is NOT (codon.c:758-760,802-804: the set is looked up for the
   character as it stands) */
VSA_SFHD uint32_t vsa_sf_base(uint32_t cls, int forward)
{
  const uint32_t b = vsa_sf_smallest(cls);
  return (vsa_sf_isplain(cls) && !forward) ? (b ^ 2u) : b;
}

/*
  codon2amino (codon.c:708-870): the amino-acid LETTER of the codon whose
  characters, in reading order, have the classes c0 c1 c2 (all != 0); aminos
  = the 64 letters of the translation table.  A wildcard in position 2 gives
  the letter all its bases agree on (equivalentbits, codon.c:605-668) and
  else its smallest base.
*/
VSA_SFHD uint8_t vsa_sf_codon(const uint8_t *aminos, int forward, uint32_t c0,
                              uint32_t c1, uint32_t c2)
{
  const uint32_t code2 = vsa_sf_base(c0, forward) << 4 |
                         vsa_sf_base(c1, forward) << 2;

  if (!vsa_sf_isplain(c2))
  {
    uint32_t b, seen = 0;
    uint8_t aa = 0;
    int agree = 1;
    for (b = 0; b < 4; b++)
    {
      if (c2 & (1u << b))
      {
        if (seen && aminos[code2 + b] != aa)
        {
          agree = 0;
        }
        if (!seen)
        {
          aa = aminos[code2 + b];
          seen = 1;
        }
      }
    }
    if (agree)
    {
      return aa;
    }
  }
  return aminos[code2 + vsa_sf_base(c2, forward)];
}

/* ---- the translation tables: the NCBI genetic codes 1-6, 9-16, 21-23 ------
   The standard code, and for every other table the codons that differ from
   it (codon code, letter). */
#define VSA_SF_STANDARD \
  "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
#define VSA_SF_TGA 14
#define VSA_SF_TAA 10
#define VSA_SF_TAG 11
#define VSA_SF_ATA 34
#define VSA_SF_AAA 42
#define VSA_SF_AGA 46
#define VSA_SF_AGG 47

typedef struct
{
  uint8_t transnum, codon, amino;
} vsa_sf_change;

static const vsa_sf_change vsa_sf_changes[] = {
    {2, VSA_SF_TGA, 'W'}, {2, VSA_SF_ATA, 'M'}, {2, VSA_SF_AGA, '*'},
    {2, VSA_SF_AGG, '*'},
    {3, VSA_SF_TGA, 'W'}, {3, VSA_SF_ATA, 'M'}, {3, 16, 'T'}, {3, 17, 'T'},
    {3, 18, 'T'}, {3, 19, 'T'}, /* CTN */
    {4, VSA_SF_TGA, 'W'},
    {5, VSA_SF_TGA, 'W'}, {5, VSA_SF_ATA, 'M'}, {5, VSA_SF_AGA, 'S'},
    {5, VSA_SF_AGG, 'S'},
    {6, VSA_SF_TAA, 'Q'}, {6, VSA_SF_TAG, 'Q'},
    {9, VSA_SF_TGA, 'W'}, {9, VSA_SF_AAA, 'N'}, {9, VSA_SF_AGA, 'S'},
    {9, VSA_SF_AGG, 'S'},
    {10, VSA_SF_TGA, 'C'},
    /* 11: the standard code (its start codons differ, which play no role) */
    {12, 19, 'S'}, /* CTG */
    {13, VSA_SF_TGA, 'W'}, {13, VSA_SF_ATA, 'M'}, {13, VSA_SF_AGA, 'G'},
    {13, VSA_SF_AGG, 'G'},
    {14, VSA_SF_TGA, 'W'}, {14, VSA_SF_TAA, 'Y'}, {14, VSA_SF_AAA, 'N'},
    {14, VSA_SF_AGA, 'S'}, {14, VSA_SF_AGG, 'S'},
    {15, VSA_SF_TAG, 'Q'},
    {16, VSA_SF_TAG, 'L'},
    {21, VSA_SF_TGA, 'W'}, {21, VSA_SF_ATA, 'M'}, {21, VSA_SF_AAA, 'N'},
    {21, VSA_SF_AGA, 'S'}, {21, VSA_SF_AGG, 'S'},
    {22, 6, '*'}, /* TCA */
    {22, VSA_SF_TAG, 'L'},
    {23, 2, '*'}, /* TTA */
};

/* checktransnum, codon.c:219-229 */
static inline int vsa_sf_transnum_ok(uint32_t transnum)
{
  return transnum >= 1 && transnum <= 23 && transnum != 7 && transnum != 8 &&
         !(transnum >= 17 && transnum <= 20);
}

/* the 64 letters of table transnum (vsa_sf_transnum_ok) */
static inline void vsa_sf_aminos(uint32_t transnum, uint8_t aminos[64])
{
  static const char standard[] = VSA_SF_STANDARD;
  uint32_t i;

  for (i = 0; i < 64; i++)
  {
    aminos[i] = (uint8_t) standard[i];
  }
  for (i = 0; i < sizeof vsa_sf_changes / sizeof vsa_sf_changes[0]; i++)
  {
    if (vsa_sf_changes[i].transnum == transnum)
    {
      aminos[vsa_sf_changes[i].codon] = vsa_sf_changes[i].amino;
    }
  }
}

/* ---- frames ----------------------------------------------------------------
   DNA sequence s of len characters becomes the sequences 6 s .. 6 s + 5:
   forward frame f = 0, 1, 2 reads the codons at f, f + 3, ..; reverse frame r
   (sequence 6 s + 3 + r) reads codon k from the characters at len - 1 - r -
   3 k, one below and two below, complemented.  Both have (len - f) / 3
   symbols, 0 where len < f (translateDNAforward / backward,
   codon.c:939-999). */
VSA_SFHD uint64_t vsa_sf_framelength(uint64_t len, uint32_t frame)
{
  const uint64_t f = frame % 3u;
  return len >= f ? (len - f) / 3u : 0;
}

/* symbols of the six frames of one sequence with a separator behind each */
VSA_SFHD uint64_t vsa_sf_span(uint64_t len)
{
  return 2u * (vsa_sf_framelength(len, 0) + vsa_sf_framelength(len, 1) +
               vsa_sf_framelength(len, 2)) + VSA_SF_FRAMES;
}

/* where frame `frame` of a sequence starts whose frame 0 starts at base */
VSA_SFHD uint64_t vsa_sf_framestart(uint64_t base, uint64_t len,
                                    uint32_t frame)
{
  uint32_t i;
  for (i = 0; i < frame; i++)
  {
    base += vsa_sf_framelength(len, i) + 1;
  }
  return base;
}

/* The codons of all six frames lie on the three grids g = 0, 1, 2 of the
   forward strand: the one at g + 3 j is symbol j of forward frame g and
   symbol (len - r) / 3 - 1 - j of the reverse frame r = (len - g) mod 3. */
VSA_SFHD uint32_t vsa_sf_reverseframe(uint64_t len, uint32_t grid)
{
  return (uint32_t) ((len + 3u - grid) % 3u);
}

/* ---- sixframeconvertmatch (sixframe.c:232-264) with procfinal.c:262-289 ----
   A record the engine delivered on the six-frame batch, q = its queryseq
   counted inside the batch, dnalen = the length of DNA sequence q / 6 ->
   the record in DNA coordinates of the forward strand: length2 = 3 length,
   seqnum2 = q / 6, relpos2; dbstart stays.  *reverse = 1 for a reverse frame
   (the flag G of the output, F otherwise).  -1: the record does not lie in
   its frame. */
VSA_SFHD int vsa_sf_convert(const vsa_match *in, uint64_t q, uint64_t dnalen,
                            uint64_t dnaoffset, vsa_match *out,
                            uint8_t *reverse)
{
  const uint32_t frame = (uint32_t) (q % VSA_SF_FRAMES);
  const uint64_t last = in->querystart + in->length;

  if (last < in->length || last > vsa_sf_framelength(dnalen, frame))
  {
    return -1;
  }
  out->length = 3u * in->length;
  out->dbstart = in->dbstart;
  out->queryseq = dnaoffset + q / VSA_SF_FRAMES;
  if (frame < 3u)
  {
    out->querystart = 3u * in->querystart + frame;
    *reverse = 0;
  } else
  {
    out->querystart = dnalen - 3u * last - (frame - 3u);
    *reverse = 1;
  }
  return 0;
}

#endif
