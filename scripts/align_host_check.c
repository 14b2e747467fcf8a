/*
  vsa_align_host and vsa_align_format on a match list written out as text, as
  a program of its own: for runs of the host code under a sanitizer
  (tests/test_align_host.py builds it with -fsanitize=address,undefined
  together with vstree_amd/csrc/align_host.c and match_sink.c).  No GPU, no
  Python in the process.  Every array has exactly the size the entries are
  told, so that a read beyond one is seen.  The scripts are made twice: once
  into no room at all, which must fail with -3 and the offsets, then into a
  buffer of exactly offsets[n] words.

  input:  kind palindromic n nsymbols nq nrecords linewidth threads
          n symbols of the text
          nsymbols symbols of the batch
          nq lines: start length
          nrecords lines: length dbstart queryseq querystart
  output: the offsets, the words, then the formatted text (original
          characters: a c g t for 0 .. 3, n for a wildcard)
*/
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"

static char errbuf[1024];

char *vsa_errbuf(void)
{
  return errbuf;
}

static uint8_t *readsymbols(FILE *f, uint64_t n, uint8_t **orig)
{
  uint8_t *s = malloc(n > 0 ? n : 1);
  uint64_t i;

  *orig = malloc(n > 0 ? n : 1);
  for (i = 0; i < n; i++)
  {
    unsigned v;
    if (fscanf(f, "%u", &v) != 1)
    {
      exit(2);
    }
    s[i] = (uint8_t) v;
    (*orig)[i] = v < 4 ? (uint8_t) "acgt"[v] : v == VSA_WILDCARD ? 'n' : 255;
  }
  return s;
}

int main(int argc, char **argv)
{
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;
  int kind, palindromic, threads, rc;
  unsigned long n, nsymbols, nq, nrecords, linewidth, i;
  uint8_t *text, *origtext, *qsym, *qorig;
  uint64_t *qstart, *qlength, *offsets;
  uint16_t *eops;
  vsa_match *rec;
  vsa_sinkparams lay;
  vsa_sink *sink = NULL;
  char *out;
  int64_t got;
  uint64_t cap;

  if (f == NULL || fscanf(f, "%d %d %lu %lu %lu %lu %lu %d", &kind,
                          &palindromic, &n, &nsymbols, &nq, &nrecords,
                          &linewidth, &threads) != 8)
  {
    return 2;
  }
  text = readsymbols(f, n, &origtext);
  qsym = readsymbols(f, nsymbols, &qorig);
  qstart = malloc((nq > 0 ? nq : 1) * 8);
  qlength = malloc((nq > 0 ? nq : 1) * 8);
  for (i = 0; i < nq; i++)
  {
    unsigned long a, b;
    if (fscanf(f, "%lu %lu", &a, &b) != 2)
    {
      return 2;
    }
    qstart[i] = a;
    qlength[i] = b;
  }
  rec = malloc((nrecords > 0 ? nrecords : 1) * sizeof *rec);
  for (i = 0; i < nrecords; i++)
  {
    unsigned long a, b, c, d;
    if (fscanf(f, "%lu %lu %lu %lu", &a, &b, &c, &d) != 4)
    {
      return 2;
    }
    rec[i].length = a;
    rec[i].dbstart = b;
    rec[i].queryseq = c;
    rec[i].querystart = d;
  }
  fclose(f);
  memset(&lay, 0, sizeof lay);
  lay.kind = kind;
  lay.palindromic = palindromic;
  lay.numofchars = 4;
  lay.threads = threads;
  lay.totallength = n;
  lay.numofsequences = 1;
  lay.numofqueries = nq;
  lay.querytotallength = nsymbols;
  lay.querystart = qstart;
  lay.querylength = qlength;
  offsets = malloc((nrecords + 1) * 8);
  rc = vsa_align_host(&lay, text, nq > 0 ? qsym : NULL, rec, nrecords,
                      palindromic, threads, offsets, NULL, 0);
  if (rc != (nrecords > 0 ? -3 : 0))
  {
    fprintf(stderr, "%d %s\n", rc, errbuf);
    return 1;
  }
  eops = malloc((offsets[nrecords] > 0 ? offsets[nrecords] : 1) * 2);
  rc = vsa_align_host(&lay, text, nq > 0 ? qsym : NULL, rec, nrecords,
                      palindromic, threads, offsets, eops, offsets[nrecords]);
  if (rc != 0)
  {
    fprintf(stderr, "%d %s\n", rc, errbuf);
    return 1;
  }
  for (i = 0; i <= nrecords; i++)
  {
    printf("%lu ", (unsigned long) offsets[i]);
  }
  printf("\n");
  for (i = 0; i < offsets[nrecords]; i++)
  {
    printf("%u ", (unsigned) eops[i]);
  }
  printf("\n");
  if (vsa_sink_open(&lay, &sink) != 0)
  {
    fprintf(stderr, "%s\n", errbuf);
    return 1;
  }
  /* too small first, then exactly what it takes */
  cap = 64;
  out = malloc(cap);
  while ((got = vsa_align_format(sink, rec, nrecords, offsets, eops, text,
                                 origtext, nq > 0 ? qsym : NULL,
                                 nq > 0 ? qorig : NULL, (uint32_t) linewidth,
                                 out, cap)) == -3)
  {
    free(out);
    cap *= 2;
    out = malloc(cap);
  }
  if (got < 0)
  {
    fprintf(stderr, "%ld %s\n", (long) got, errbuf);
    return 1;
  }
  fwrite(out, 1, (size_t) got, stdout);
  vsa_sink_close(sink);
  free(out);
  free(eops);
  free(offsets);
  free(rec);
  free(qstart);
  free(qlength);
  free(text);
  free(origtext);
  free(qsym);
  free(qorig);
  return 0;
}
