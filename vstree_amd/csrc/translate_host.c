/* Host side of the six-frame translation (include/vstree_amd.h, vmatch
   -dnavsprot): the translation of a DNA Multiseq into the protein Multiseq
   of its six reading frames and the conversion of match records back to DNA
   coordinates, both by the rules of sixframe_rules.h.  No GPU involved; the
   kernels of translate.hip are checked against this. */
#include <stdio.h>
#include <string.h>
#include "vstree_amd.h"
#include "sixframe_rules.h"

#include "host_common.h"

int vsa_transnum_check(uint32_t transnum)
{
  if (!vsa_sf_transnum_ok(transnum))
  {
    /* checktransnum, kurtz/codon.c:219-229 */
    return vsa_fail(-2, "illegal translation table number %lu: must be "
                        "number in the range [1,23] except for 7, 8, 17, 18, "
                        "19 and 20",
                        (unsigned long) transnum);
  }
  return 0;
}

/* alpha.mapsize - 1 of a symbol map: the codes below VSA_UNDEFBWT in use */
static uint32_t numofcharsof(const uint8_t symbolmap[256])
{
  uint32_t i, nc = 0;

  for (i = 0; i < 256; i++)
  {
    if (symbolmap[i] < VSA_UNDEFBWT && symbolmap[i] + 1u > nc)
    {
      nc = symbolmap[i] + 1u;
    }
  }
  return nc;
}

/* one codon: 0 and the mapped symbol, or -2 and the message */
static int codon(const uint8_t *aminos, const uint8_t symbolmap[256],
                 uint32_t numofchars, int forward, uint8_t ch0, uint8_t ch1,
                 uint8_t ch2, uint8_t *symbol)
{
  const uint32_t c0 = vsa_sf_class(ch0), c1 = vsa_sf_class(ch1),
                 c2 = vsa_sf_class(ch2);
  uint8_t aa, code;

  if (c0 == 0 || c1 == 0 || c2 == 0)
  {
    /* ILLEGALCHAR, kurtz/codon.c:42-44 */
    const int which = c0 == 0 ? 0 : (c1 == 0 ? 1 : 2);
    const uint8_t ch = which == 0 ? ch0 : (which == 1 ? ch1 : ch2);
    return vsa_fail(-2, "illegal char c%d='%c'(%lu)", which,
                        ch, (unsigned long) ch);
  }
  aa = vsa_sf_codon(aminos, forward, c0, c1, c2);
  code = symbolmap[aa];
  if (code >= numofchars && code <= VSA_UNDEFBWT)
  {
    return vsa_fail(-2, "amino acid '%c' of the translation has the code "
                        "%lu, which is no symbol of the alphabet of %lu "
                        "characters", aa, (unsigned long) code,
                        (unsigned long) numofchars);
  }
  *symbol = code;
  return 0;
}

int vsa_translate_host(uint32_t transnum, const uint8_t *dnachars,
                       uint64_t nchars, const uint64_t *start,
                       const uint64_t *length, uint64_t nq,
                       const uint8_t symbolmap[256], uint8_t *protein,
                       uint64_t capacity, uint64_t *pstart, uint64_t *plength,
                       uint64_t *nsymbols)
{
  uint8_t aminos[64];
  uint64_t s, pos = 0, need = 0;
  uint32_t numofchars;

  if (nsymbols != NULL)
  {
    *nsymbols = 0;
  }
  if (symbolmap == NULL || nsymbols == NULL ||
      (nq > 0 && (start == NULL || length == NULL || pstart == NULL ||
                  plength == NULL)) ||
      (nchars > 0 && dnachars == NULL))
  {
    return vsa_fail(-1, "vsa_translate_host: NULL argument");
  }
  if (vsa_transnum_check(transnum) != 0)
  {
    return -2;
  }
  for (s = 0; s < nq; s++)
  {
    if (start[s] > nchars || length[s] > nchars - start[s])
    {
      return vsa_fail(-2, "sequence %lu [%lu, +%lu) lies outside the "
                          "buffer of %lu characters", (unsigned long) s,
                          (unsigned long) start[s], (unsigned long) length[s],
                          (unsigned long) nchars);
    }
    need += vsa_sf_span(length[s]);
  }
  need -= nq > 0 ? 1 : 0; /* no separator behind the last frame */
  if (need > capacity || (need > 0 && protein == NULL))
  {
    return vsa_fail(-3, "vsa_translate_host: %lu symbols do "
                        "not fit a buffer of %lu", (unsigned long) need,
                        (unsigned long) capacity);
  }
  vsa_sf_aminos(transnum, aminos);
  numofchars = numofcharsof(symbolmap);
  /* the order of singlesixframetranslateDNA (kurtz/sixframe.c:70-143): the
     first error met is the reference's */
  for (s = 0; s < nq; s++)
  {
    const uint8_t *dna = dnachars + start[s];
    const uint64_t len = length[s];
    uint32_t frame;

    for (frame = 0; frame < VSA_SF_FRAMES; frame++)
    {
      const uint64_t n = vsa_sf_framelength(len, frame);
      const uint32_t f = frame % 3u;
      uint64_t k;

      pstart[VSA_SF_FRAMES * s + frame] = pos;
      plength[VSA_SF_FRAMES * s + frame] = n;
      for (k = 0; k < n; k++)
      {
        int rc;
        if (frame < 3u)
        {
          const uint8_t *c = dna + f + 3u * k;
          rc = codon(aminos, symbolmap, numofchars, 1, c[0], c[1], c[2],
                     protein + pos);
        } else
        {
          const uint8_t *c = dna + (len - 1u - f - 3u * k);
          rc = codon(aminos, symbolmap, numofchars, 0, c[0], *(c - 1),
                     *(c - 2), protein + pos);
        }
        if (rc != 0)
        {
          return rc;
        }
        pos++;
      }
      if (pos < need)
      {
        protein[pos++] = (uint8_t) VSA_SEPARATOR;
      }
    }
  }
  *nsymbols = need;
  return 0;
}

int vsa_translated_convert_host(const vsa_match *matches, uint64_t n,
                                const uint64_t *dnalength, uint64_t numofdna,
                                uint64_t offset, vsa_match *queryview,
                                uint8_t *reverse)
{
  uint64_t i;

  if ((n > 0 && (matches == NULL || queryview == NULL)) ||
      (numofdna > 0 && dnalength == NULL))
  {
    return vsa_fail(-1, "vsa_translated_convert_host: NULL argument");
  }
  if (offset % VSA_SF_FRAMES != 0)
  {
    return vsa_fail(-2, "the offset %lu of a six-frame batch "
                        "is no multiple of 6", (unsigned long) offset);
  }
  for (i = 0; i < n; i++)
  {
    const uint64_t q = matches[i].queryseq - offset;
    uint8_t rev = 0;
    vsa_match out;

    if (matches[i].queryseq < offset || q / VSA_SF_FRAMES >= numofdna ||
        vsa_sf_convert(matches + i, q, dnalength[q / VSA_SF_FRAMES],
                       offset / VSA_SF_FRAMES, &out, &rev) != 0)
    {
      return vsa_fail(-2, "record %lu does not lie in a "
                          "frame of the %lu DNA sequences", (unsigned long) i,
                          (unsigned long) numofdna);
    }
    queryview[i] = out;
    if (reverse != NULL)
    {
      reverse[i] = rev;
    }
  }
  return 0;
}
