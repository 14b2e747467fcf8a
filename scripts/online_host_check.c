/*
  vsa_findcompletematches_online_host on a text and a batch written out as
  text, as a program of its own: for runs of the host code under a sanitizer
  (tests/test_online_host.py builds it with -fsanitize=address,undefined
  together with vstree_amd/csrc/online_host.c).  No GPU, no Python in the
  process.  Text and queries lie in allocations of their exact sizes, so a
  read beyond them is seen.  The batch is scanned twice, cut into slices over
  `threads` threads and unsliced on one thread, and the two lists must be
  equal; before that the word comparison of online_rules.h is compared with a
  loop over the bytes.  The batches the test writes out include a text of low
  complexity (every position a start position), texts of 7 and 9 symbols
  with reads longer than the text under a percent threshold, and the empty
  text: n = 0 and reads of any length are taken.

  input:  n nsymbols nq mode K percent remred threads
          n symbols of the text
          nsymbols symbols of the batch
          nq lines: start length
  output: one line per match: length dbstart queryseq distance
*/
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"
#include "online_rules.h"

static char errbuf[1024];

char *vsa_errbuf(void)
{
  return errbuf;
}

static uint64_t rngstate = 88172645463325252ull;

static uint64_t rnd(void)
{
  rngstate ^= rngstate << 13;
  rngstate ^= rngstate >> 7;
  rngstate ^= rngstate << 17;
  return rngstate;
}

static int checkwords(void)
{
  static const uint8_t alphabet[] = {0, 1, 2, 3, 253, VSA_WILDCARD,
                                     VSA_SEPARATOR};
  int round;

  for (round = 0; round < 200000; round++)
  {
    uint8_t t[8], p[8];
    uint64_t tw, pw;
    const uint32_t count = 1 + (uint32_t) (rnd() % 8);
    const int mode = (rnd() & 1) ? VSA_ONLINE_EXACT : VSA_ONLINE_HAMMING;
    uint32_t i, mm = 0;
    int barred = 0, got;

    for (i = 0; i < 8; i++)
    {
      t[i] = alphabet[rnd() % (rnd() % 3 ? 4 : sizeof alphabet)];
      p[i] = (rnd() & 3) ? t[i] : alphabet[rnd() % sizeof alphabet];
    }
    for (i = 0; i < count; i++)
    {
      mm += t[i] != p[i];
      barred |= mode == VSA_ONLINE_EXACT ? t[i] >= VSA_WILDCARD
                                         : t[i] == VSA_SEPARATOR;
    }
    memcpy(&tw, t, 8);
    memcpy(&pw, p, 8);
    if (vsa_online_word(tw, pw, count, mode, &got) != mm || got != barred)
    {
      fprintf(stderr, "round %d: the word comparison differs from the loop "
              "over the bytes\n", round);
      return -1;
    }
  }
  return 0;
}

static int readsymbols(FILE *f, uint8_t *out, unsigned long n)
{
  unsigned long i, v;

  for (i = 0; i < n; i++)
  {
    if (fscanf(f, "%lu", &v) != 1 || v > 255)
    {
      return -1;
    }
    out[i] = (uint8_t) v;
  }
  return 0;
}

int main(int argc, char **argv)
{
  unsigned long n, nsym, nq, mode, K, percent, remred, threads, i, v[2];
  const uint64_t capacity = 1 << 20;
  uint8_t *text, *symbols;
  uint64_t *qstart, *qlen, nout = 0, nout2 = 0;
  vsa_match *out, *out2;
  int rc;
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;

  if (checkwords() != 0)
  {
    return 3;
  }
  if (f == NULL || fscanf(f, "%lu %lu %lu %lu %lu %lu %lu %lu", &n, &nsym,
                          &nq, &mode, &K, &percent, &remred, &threads) != 8)
  {
    fprintf(stderr, "usage: %s batch.txt\n", argv[0]);
    return 2;
  }
  text = malloc(n > 0 ? n : 1);
  symbols = malloc(nsym > 0 ? nsym : 1);
  qstart = malloc((nq + 1) * sizeof *qstart);
  qlen = malloc((nq + 1) * sizeof *qlen);
  out = malloc(capacity * sizeof *out);
  out2 = malloc(capacity * sizeof *out2);
  if (readsymbols(f, text, n) != 0 || readsymbols(f, symbols, nsym) != 0)
  {
    return 2;
  }
  for (i = 0; i < nq; i++)
  {
    if (fscanf(f, "%lu %lu", &v[0], &v[1]) != 2)
    {
      return 2;
    }
    qstart[i] = v[0];
    qlen[i] = v[1];
  }
  fclose(f);
  rc = vsa_findcompletematches_online_host(text, n, symbols, qstart, qlen, nq,
                                           0, (int) mode, K, (int) percent,
                                           (int) remred, (int) threads, out,
                                           capacity, &nout);
  if (rc != 0)
  {
    fprintf(stderr, "%d: %s\n", rc, vsa_errbuf());
  } else
  {
    rc = vsa_findcompletematches_online_host(text, n, symbols, qstart, qlen,
                                             nq, 0, (int) mode, K,
                                             (int) percent, (int) remred, 1,
                                             out2, capacity, &nout2);
    if (rc == 0 && (nout != nout2 ||
                    memcmp(out, out2, nout * sizeof *out) != 0))
    {
      fprintf(stderr, "sliced: %lu matches, unsliced: %lu, or other ones\n",
              (unsigned long) nout, (unsigned long) nout2);
      rc = 4;
    }
  }
  for (i = 0; i < nout; i++)
  {
    printf("%lu %lu %lu %lu\n", (unsigned long) out[i].length,
           (unsigned long) out[i].dbstart, (unsigned long) out[i].queryseq,
           (unsigned long) out[i].querystart);
  }
  free(text);
  free(symbols);
  free(qstart);
  free(qlen);
  free(out);
  free(out2);
  return rc != 0;
}
