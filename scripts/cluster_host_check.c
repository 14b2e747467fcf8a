/*
  vsa_cluster_host on a list written out as text, as a program of its own:
  for runs of the host code under a sanitizer (tests/test_cluster_host.py
  builds it with -fsanitize=address,undefined together with
  vstree_amd/csrc/cluster_host.c).  No GPU, no Python in the process.

  input:  totallength numofsequences percsmall perclarge n
          numofsequences - 1 separator positions
          n lines: length dbstart queryseq querystart palindromic
  output: the lines vmatch prints, then one line per cluster
          "edges c: r r r" with the records of its match file
*/
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "vstree_amd.h"

static char errbuf[1024];

char *vsa_errbuf(void)
{
  return errbuf;
}

int main(int argc, char **argv)
{
  unsigned long total, nseq, small, large, n, i, c, v[5];
  uint64_t *markpos, *edgestart, *edgerecord;
  vsa_match *rec;
  uint8_t *flags;
  vsa_sinkparams layout = {0};
  vsa_clusterparams params;
  vsa_clusterstats st;
  char *text;
  int64_t written = 0;
  uint64_t cap;
  int rc;
  FILE *f = argc > 1 ? fopen(argv[1], "r") : NULL;

  if (f == NULL || fscanf(f, "%lu %lu %lu %lu %lu", &total, &nseq, &small,
                          &large, &n) != 5 || nseq < 1)
  {
    fprintf(stderr, "usage: %s list.txt\n", argv[0]);
    return 2;
  }
  markpos = malloc(nseq * sizeof *markpos);
  rec = malloc((n + 1) * sizeof *rec);
  flags = malloc(n + 1);
  edgestart = malloc((nseq / 2 + 2) * sizeof *edgestart);
  edgerecord = malloc((n + 1) * sizeof *edgerecord);
  cap = 512 + 64 * (nseq / 2 + 2) + 22 * (nseq + 1);
  text = malloc(cap);
  for (i = 0; i + 1 < nseq; i++)
  {
    if (fscanf(f, "%lu", &v[0]) != 1)
    {
      return 2;
    }
    markpos[i] = v[0];
  }
  for (i = 0; i < n; i++)
  {
    if (fscanf(f, "%lu %lu %lu %lu %lu", &v[0], &v[1], &v[2], &v[3],
               &v[4]) != 5)
    {
      return 2;
    }
    rec[i].length = v[0];
    rec[i].dbstart = v[1];
    rec[i].queryseq = v[2];
    rec[i].querystart = v[3];
    flags[i] = (uint8_t) v[4];
  }
  fclose(f);
  layout.kind = VSA_SINK_SELF;
  layout.totallength = total;
  layout.numofsequences = nseq;
  layout.markpos = markpos;
  params.percsmall = (uint32_t) small;
  params.perclarge = (uint32_t) large;
  rc = vsa_cluster_host(&layout, &params, rec, flags, n, &st, NULL, NULL, NULL,
                        edgestart, edgerecord, text, cap, &written);
  if (rc != 0)
  {
    fprintf(stderr, "error %d: %s\n", rc, errbuf);
  } else
  {
    fwrite(text, 1, (size_t) written, stdout);
    for (c = 0; c < st.clusters; c++)
    {
      printf("edges %lu:", c);
      for (i = edgestart[c]; i < edgestart[c + 1]; i++)
      {
        printf(" %lu", (unsigned long) edgerecord[i]);
      }
      printf("\n");
    }
  }
  free(markpos);
  free(rec);
  free(flags);
  free(edgestart);
  free(edgerecord);
  free(text);
  return rc == 0 ? 0 : 1;
}
