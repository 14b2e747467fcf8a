/*
  vsa_extend_hamming_host on a seed list written out as text, as a program of
  its own: for runs of the host code under a sanitizer
  (tests/test_extend_host.py builds it with -fsanitize=address,undefined
  together with vstree_amd/csrc/extend_host.c and match_sink.c).  No GPU, no
  Python in the process.  Before it reads anything it compares the word
  arithmetic of extend_rules.h (vsa_ext_marks8) with the symbols taken one by
  one, on words made of ordinary symbols, wildcards and separators.

  input:  n nsymbols nq nseeds L K S threads     (nq = 0: a self layout)
          n symbols of the text
          nsymbols symbols of the batch
          nq lines: start length
          nseeds lines: length dbstart queryseq querystart
  output: one line per match: length distance dbstart queryseq querystart
*/
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "extend_rules.h"

static char errbuf[1024];

char *vsa_errbuf(void)
{
  return errbuf;
}

static int checkwords(void)
{
  static const uint8_t alphabet[] = {0, 1, 2, 3, 19, 127, 128, 252, 253,
                                     VSA_WILDCARD, VSA_SEPARATOR};
  uint64_t x = 88172645463325252ull;
  int round, k;

  for (round = 0; round < 200000; round++)
  {
    uint64_t a = 0, b = 0;
    uint32_t marks, sep, wantmarks = 0, wantsep = 0;
    for (k = 0; k < 8; k++)
    {
      uint8_t ca, cb;
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      ca = alphabet[x % sizeof alphabet];
      cb = (x >> 20) % 3 == 0 ? alphabet[(x >> 8) % sizeof alphabet] : ca;
      a |= (uint64_t) ca << (8 * k);
      b |= (uint64_t) cb << (8 * k);
      if (ca != cb || ca >= VSA_WILDCARD)
      {
        wantmarks |= 1u << k;
      }
      if (ca == VSA_SEPARATOR || cb == VSA_SEPARATOR)
      {
        wantsep |= 1u << k;
      }
    }
    marks = vsa_ext_marks8(a, b, &sep);
    if (marks != wantmarks || sep != wantsep)
    {
      fprintf(stderr, "vsa_ext_marks8(%016lx, %016lx): %02x/%02x, not "
              "%02x/%02x\n", (unsigned long) a, (unsigned long) b, marks, sep,
              wantmarks, wantsep);
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
  unsigned long n, nsym, nq, nseeds, L, K, S, threads, i, v[4];
  uint8_t *text, *symbols;
  uint64_t *qstart, *qlen, nout = 0;
  vsa_match *seeds, *out;
  vsa_sinkparams layout = {0};
  int rc;
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;

  if (checkwords() != 0)
  {
    return 3;
  }
  if (f == NULL || fscanf(f, "%lu %lu %lu %lu %lu %lu %lu %lu", &n, &nsym,
                          &nq, &nseeds, &L, &K, &S, &threads) != 8)
  {
    fprintf(stderr, "usage: %s seeds.txt\n", argv[0]);
    return 2;
  }
  text = malloc(n + 1);
  symbols = malloc(nsym + 1);
  qstart = malloc((nq + 1) * sizeof *qstart);
  qlen = malloc((nq + 1) * sizeof *qlen);
  seeds = malloc((nseeds + 1) * sizeof *seeds);
  out = malloc((nseeds + 1) * sizeof *out);
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
  for (i = 0; i < nseeds; i++)
  {
    if (fscanf(f, "%lu %lu %lu %lu", &v[0], &v[1], &v[2], &v[3]) != 4)
    {
      return 2;
    }
    seeds[i].length = v[0];
    seeds[i].dbstart = v[1];
    seeds[i].queryseq = v[2];
    seeds[i].querystart = v[3];
  }
  fclose(f);
  layout.kind = nq > 0 ? VSA_SINK_QUERY : VSA_SINK_SELF;
  layout.numofchars = 4;
  layout.totallength = n;
  layout.numofsequences = 1;
  layout.numofqueries = nq;
  layout.querystart = qstart;
  layout.querylength = qlen;
  rc = vsa_extend_hamming_host(&layout, text, nq > 0 ? symbols : NULL, seeds,
                               nseeds, L, K, S, (int) threads, out, nseeds,
                               &nout);
  if (rc != 0)
  {
    fprintf(stderr, "%d: %s\n", rc, vsa_errbuf());
  }
  for (i = 0; i < nout; i++)
  {
    printf("%lu %lu %lu %lu %lu\n",
           (unsigned long) VSA_HAMMING_LENGTH(out[i].length),
           (unsigned long) VSA_HAMMING_DISTANCE(out[i].length),
           (unsigned long) out[i].dbstart, (unsigned long) out[i].queryseq,
           (unsigned long) out[i].querystart);
  }
  free(text);
  free(symbols);
  free(qstart);
  free(qlen);
  free(seeds);
  free(out);
  return rc != 0;
}
