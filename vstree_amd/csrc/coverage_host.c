/* Host side of the match coverage (include/vstree_amd.h): the reference's
   output of the unmarked regions (shownomatch, Vmatch/nomatch.c:36-135) and
   its masking of the marked characters (showmaskedseq,
   Vmatch/showmasked.c:49-153).  No GPU involved. */
#include <ctype.h>
#include <stdio.h>
#include <string.h>
#include "vstree_amd.h"
#include "host_common.h"

int64_t vsa_nomatch_format(const vsa_match *intervals, uint64_t n,
                           uint32_t showmode, uint64_t posoffset,
                           char *buffer, uint64_t capacity)
{
  uint64_t used = 0, i;

  if ((intervals == NULL && n > 0) || (buffer == NULL && capacity > 0))
  {
    return vsa_fail(-1, "vsa_nomatch_format: NULL argument");
  }
  for (i = 0; i < n; i++)
  {
    char line[80];
    int len;
    const uint64_t start = intervals[i].dbstart - posoffset;

    if (showmode & VSA_SHOW_ABSOLUTE)
    {
      len = snprintf(line, sizeof line, ">%lu %lu\n", (unsigned long) start,
                     (unsigned long) intervals[i].length);
    } else if (posoffset != 0)
    {
      /* the query part of an index with queries: seqnum and seqnumstart of
         nomatchsubstringsout (nomatch.c:186,226-238) stay 0 */
      len = snprintf(line, sizeof line, ">0 %lu %lu\n", (unsigned long) start,
                     (unsigned long) intervals[i].length);
    } else
    {
      len = snprintf(line, sizeof line, ">%lu %lu %lu\n",
                     (unsigned long) intervals[i].queryseq,
                     (unsigned long) intervals[i].querystart,
                     (unsigned long) intervals[i].length);
    }
    if (used + (uint64_t) len > capacity)
    {
      return vsa_fail(-2, "vsa_nomatch_format: buffer of %lu bytes is too "
                      "small", (unsigned long) capacity);
    }
    memcpy(buffer + used, line, (size_t) len);
    used += (uint64_t) len;
  }
  return (int64_t) used;
}

int vsa_mask_apply(const uint64_t *bits, uint64_t nbits, uint8_t *chars,
                   int maskchar, uint64_t *masked)
{
  uint64_t i, count = 0;

  if ((bits == NULL || chars == NULL) && nbits > 0)
  {
    return vsa_fail(-1, "vsa_mask_apply: NULL argument");
  }
  for (i = 0; i < nbits; i++)
  {
    const uint8_t c = chars[i];

    if (c == VSA_SEPARATOR || !((bits[i >> 6] >> (i & 63)) & 1u))
    {
      continue;
    }
    count++;
    if (maskchar == VSA_MASK_TOUPPER)
    {
      if (islower(c))
      {
        chars[i] = (uint8_t) toupper(c);
      } else if (c != '*')
      {
        return vsa_fail(-4, "cannot convert character %c to %s case", c,
                        "upper");
      }
    } else if (maskchar == VSA_MASK_TOLOWER)
    {
      if (isupper(c))
      {
        chars[i] = (uint8_t) tolower(c);
      } else if (c != '*')
      {
        return vsa_fail(-4, "cannot convert character %c to %s case", c,
                        "lower");
      }
    } else
    {
      chars[i] = (uint8_t) maskchar;
    }
  }
  if (masked != NULL)
  {
    *masked = count;
  }
  return 0;
}
