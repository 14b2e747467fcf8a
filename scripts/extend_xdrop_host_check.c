/*
  vsa_extend_xdrop_host on a seed list written out as text, as a program of
  its own: for runs of the host code under a sanitizer
  (tests/test_extend_xdrop_host.py builds it with -fsanitize=address,undefined
  together with vstree_amd/csrc/extend_xdrop_host.c).  No GPU, no Python in
  the process.  Before it reads anything it compares the slide of
  extend_xdrop_rules.h that looks at eight symbols per step with the one that
  takes them one by one, on arrays of ordinary symbols, wildcards and
  separators, to the right and to the left, and a whole side made both ways.
  The seed list is then extended twice, eight symbols and one symbol per
  step, and the two lists must be equal.

  input:  n nsymbols nq nseeds L X hamming S threads   (nq = 0: a self layout)
          n symbols of the text
          nsymbols symbols of the batch
          nq lines: start length
          nseeds lines: length dbstart queryseq querystart
  output: one line per match:
          length1 length2 distance dbstart queryseq querystart
*/
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"
#include "extend_xdrop_rules.h"

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

static int checkslides(void)
{
  enum { N = 96, CAP = 4 * N };
  static const uint8_t alphabet[] = {0, 1, 2, 3, 253, VSA_WILDCARD,
                                     VSA_SEPARATOR};
  uint8_t *u = malloc(N), *v = malloc(N); /* exact sizes: a read beyond is seen */
  int64_t *rows = malloc((2 * CAP + VSA_XD_RING) * sizeof *rows);
  int round, i;

  for (round = 0; round < 100000; round++)
  {
    vsa_xd_arrays a1, a2;
    vsa_xd_best b1, b2;
    int64_t i1, j1, i2, j2;
    const int left = (int) (rnd() & 1);
    const uint64_t pos1 = 1 + rnd() % (N - 6), pos2 = 1 + rnd() % (N - 6),
                   length = 1 + rnd() % 3, xdrop = 1 + rnd() % 12;
    const uint8_t common = alphabet[rnd() % 4];

    for (i = 0; i < N; i++)
    {
      /* long equal stretches with rare special symbols */
      u[i] = rnd() % 23 == 0 ? alphabet[rnd() % sizeof alphabet] : common;
      v[i] = rnd() % 23 == 0 ? alphabet[rnd() % sizeof alphabet] : common;
    }
    if (!vsa_xd_arrays_init(&a1, u, N, v, N, pos1, pos2, length, left))
    {
      continue;
    }
    a2 = a1;
    i1 = i2 = (int64_t) (rnd() % 9);
    j1 = j2 = (int64_t) (rnd() % 9);
    vsa_xd_slide(&a1, &i1, &j1, 0);
    vsa_xd_slide(&a2, &i2, &j2, 1);
    if (i1 != i2 || j1 != j2 || a1.ulen != a2.ulen || a1.vlen != a2.vlen)
    {
      fprintf(stderr, "round %d: eight symbols per step (%ld, %ld) lengths "
              "(%ld, %ld), one by one (%ld, %ld) lengths (%ld, %ld)\n", round,
              (long) i1, (long) j1, (long) a1.ulen, (long) a1.vlen, (long) i2,
              (long) j2, (long) a2.ulen, (long) a2.vlen);
      return -1;
    }
    (void) vsa_xd_arrays_init(&a1, u, N, v, N, pos1, pos2, length, left);
    a2 = a1;
    if (vsa_xd_editside(&a1, (int64_t) xdrop, rows, rows + CAP, CAP,
                        rows + 2 * CAP, 0, &b1) != 0 ||
        vsa_xd_editside(&a2, (int64_t) xdrop, rows, rows + CAP, CAP,
                        rows + 2 * CAP, 1, &b2) != 0 ||
        b1.ivalue != b2.ivalue || b1.jvalue != b2.jvalue ||
        b1.score != b2.score)
    {
      fprintf(stderr, "round %d: a side made both ways differs\n", round);
      return -1;
    }
  }
  free(u);
  free(v);
  free(rows);
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
  unsigned long n, nsym, nq, nseeds, L, X, hamming, S, threads, i, v[4];
  uint8_t *text, *symbols;
  uint64_t *qstart, *qlen, nout = 0, nout2 = 0;
  vsa_match *seeds, *out, *out2;
  vsa_sinkparams layout = {0};
  int rc;
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;

  if (checkslides() != 0)
  {
    return 3;
  }
  if (f == NULL || fscanf(f, "%lu %lu %lu %lu %lu %lu %lu %lu %lu", &n,
                          &nsym, &nq, &nseeds, &L, &X, &hamming, &S,
                          &threads) != 9)
  {
    fprintf(stderr, "usage: %s seeds.txt\n", argv[0]);
    return 2;
  }
  /* (exact sizes: a read beyond a text is seen) */
  text = malloc(n > 0 ? n : 1);
  symbols = malloc(nsym > 0 ? nsym : 1);
  qstart = malloc((nq + 1) * sizeof *qstart);
  qlen = malloc((nq + 1) * sizeof *qlen);
  seeds = malloc((nseeds + 1) * sizeof *seeds);
  out = malloc((nseeds + 1) * sizeof *out);
  out2 = malloc((nseeds + 1) * sizeof *out2);
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
  unsetenv("VSA_EXTEND_XDROP_SCALAR");
  rc = vsa_extend_xdrop_host(&layout, text, nq > 0 ? symbols : NULL, seeds,
                             nseeds, L, X, (int) hamming, S, (int) threads,
                             out, nseeds, &nout);
  if (rc != 0)
  {
    fprintf(stderr, "%d: %s\n", rc, vsa_errbuf());
  } else
  {
    setenv("VSA_EXTEND_XDROP_SCALAR", "1", 1);
    rc = vsa_extend_xdrop_host(&layout, text, nq > 0 ? symbols : NULL, seeds,
                               nseeds, L, X, (int) hamming, S, (int) threads,
                               out2, nseeds, &nout2);
    if (rc == 0 && (nout != nout2 ||
                    memcmp(out, out2, nout * sizeof *out) != 0))
    {
      fprintf(stderr, "eight symbols per step: %lu matches, one symbol per "
              "step: %lu, or other ones\n", (unsigned long) nout,
              (unsigned long) nout2);
      rc = 4;
    }
  }
  for (i = 0; i < nout; i++)
  {
    printf("%lu %lu %lu %lu %lu %lu\n",
           (unsigned long) VSA_XDROP_LENGTH1(out[i].length),
           (unsigned long) VSA_XDROP_LENGTH2(out[i].length),
           (unsigned long) VSA_XDROP_DISTANCE(out[i].querystart),
           (unsigned long) out[i].dbstart, (unsigned long) out[i].queryseq,
           (unsigned long) VSA_XDROP_START(out[i].querystart));
  }
  free(text);
  free(symbols);
  free(qstart);
  free(qlen);
  free(seeds);
  free(out);
  free(out2);
  return rc != 0;
}
