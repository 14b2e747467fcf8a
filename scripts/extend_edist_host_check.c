/*
  vsa_extend_edist_host on a seed list written out as text, as a program of
  its own: for runs of the host code under a sanitizer
  (tests/test_extend_edist_host.py builds it with -fsanitize=address,undefined
  together with vstree_amd/csrc/extend_edist_host.c and match_sink.c).  No
  GPU, no Python in the process.  Before it reads anything it compares the
  slide of extend_edist_rules.h that looks at eight symbols per step
  (vsa_ed_slide8) with the one that takes them one by one (vsa_ed_slide), on
  texts of ordinary symbols, wildcards and separators, to the right and to
  the left, under bounds of every kind, and vsa_ed_replay with a slide made
  again under tighter bounds.  The seed list is then extended twice, eight
  symbols and one symbol per step, and the two lists must be equal.

  input:  n nsymbols nq nseeds L K S threads     (nq = 0: a self layout)
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
#include "extend_edist_rules.h"

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
  enum { N = 96 };
  static const uint8_t alphabet[] = {0, 1, 2, 3, 253, VSA_WILDCARD,
                                     VSA_SEPARATOR};
  uint8_t *u = malloc(N), *v = malloc(N); /* exact sizes: a read beyond is seen */
  int round, i;

  for (round = 0; round < 100000; round++)
  {
    vsa_ed_side s;
    vsa_ed_bounds b1, b2, b3;
    int64_t t, k, m1, m2, m3;
    const int left = (int) (rnd() & 1);
    const uint64_t pos1 = rnd() % (N - 4), pos2 = rnd() % (N - 4),
                   length = 1 + rnd() % 3;
    const uint8_t common = alphabet[rnd() % 4];

    for (i = 0; i < N; i++)
    {
      /* long equal stretches with rare special symbols */
      u[i] = rnd() % 23 == 0 ? alphabet[rnd() % sizeof alphabet] : common;
      v[i] = rnd() % 23 == 0 ? alphabet[rnd() % sizeof alphabet] : common;
    }
    vsa_ed_side_init(&s, u, N, v, N, 0, pos1, pos2, length, left, 5, 1000);
    vsa_ed_bounds_init(&s, &b1);
    if (rnd() % 3 == 0 && s.ulen > 0)
    {
      b1.ub = (int64_t) (rnd() % (uint64_t) (s.ulen + 1));
    }
    if (rnd() % 3 == 0 && s.vlen > 0)
    {
      b1.vb = (int64_t) (rnd() % (uint64_t) (s.vlen + 1));
    }
    k = (int64_t) (rnd() % 11) - 5;
    t = (int64_t) (rnd() % 9);
    if (t + k < 0)
    {
      continue;
    }
    b2 = b1;
    m1 = vsa_ed_slide(&s, t, k, &b1);
    m2 = vsa_ed_slide8(&s, t, k, &b2);
    if (m1 != m2 || b1.ub != b2.ub || b1.vb != b2.vb)
    {
      fprintf(stderr, "round %d: vsa_ed_slide8 %ld (%ld, %ld), one by one "
              "%ld (%ld, %ld)\n", round, (long) m2, (long) b2.ub,
              (long) b2.vb, (long) m1, (long) b1.ub, (long) b1.vb);
      return -1;
    }
    /* the slide made under loose bounds and replayed under tight ones ==
       the slide made under the tight ones */
    {
      vsa_ed_bounds loose, tight, replayed;
      int read, seps = 0;
      vsa_ed_bounds_init(&s, &loose);
      tight = loose;
      if (tight.ub > 0)
      {
        tight.ub = (int64_t) (rnd() % (uint64_t) (tight.ub + 1));
      }
      if (tight.vb > 0 && rnd() % 2 == 0)
      {
        tight.vb = (int64_t) (rnd() % (uint64_t) (tight.vb + 1));
      }
      replayed = tight;
      b3 = loose;
      m3 = vsa_ed_slide(&s, t, k, &b3);
      read = t + m3 < loose.ub && t + m3 + k < loose.vb;
      if (read)
      {
        seps = (vsa_ed_symu(&s, t + m3) == VSA_SEPARATOR ? 1 : 0) |
               (vsa_ed_symv(&s, t + m3 + k) == VSA_SEPARATOR ? 2 : 0);
      }
      m3 = vsa_ed_replay(t, k, m3, read, seps, &replayed);
      m1 = vsa_ed_slide(&s, t, k, &tight);
      if (m1 != m3 || tight.ub != replayed.ub || tight.vb != replayed.vb)
      {
        fprintf(stderr, "round %d: vsa_ed_replay %ld (%ld, %ld), the slide "
                "%ld (%ld, %ld)\n", round, (long) m3, (long) replayed.ub,
                (long) replayed.vb, (long) m1, (long) tight.ub,
                (long) tight.vb);
        return -1;
      }
    }
  }
  free(u);
  free(v);
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
  uint64_t *qstart, *qlen, nout = 0, nout2 = 0;
  vsa_match *seeds, *out, *out2;
  vsa_sinkparams layout = {0};
  int rc;
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;

  if (checkslides() != 0)
  {
    return 3;
  }
  if (f == NULL || fscanf(f, "%lu %lu %lu %lu %lu %lu %lu %lu", &n, &nsym,
                          &nq, &nseeds, &L, &K, &S, &threads) != 8)
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
  unsetenv("VSA_EXTEND_EDIST_SCALAR");
  rc = vsa_extend_edist_host(&layout, text, nq > 0 ? symbols : NULL, seeds,
                             nseeds, L, K, S, (int) threads, out, nseeds,
                             &nout);
  if (rc != 0)
  {
    fprintf(stderr, "%d: %s\n", rc, vsa_errbuf());
  } else
  {
    setenv("VSA_EXTEND_EDIST_SCALAR", "1", 1);
    rc = vsa_extend_edist_host(&layout, text, nq > 0 ? symbols : NULL, seeds,
                               nseeds, L, K, S, (int) threads, out2, nseeds,
                               &nout2);
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
           (unsigned long) VSA_EDIST_LENGTH1(out[i].length),
           (unsigned long) VSA_EDIST_LENGTH2(out[i].length),
           (unsigned long) VSA_EDIST_DISTANCE(out[i].length),
           (unsigned long) out[i].dbstart, (unsigned long) out[i].queryseq,
           (unsigned long) out[i].querystart);
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
