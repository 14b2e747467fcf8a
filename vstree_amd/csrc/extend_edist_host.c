/* Host side of the edit-distance extension of exact seeds
   (include/vstree_amd_edist.h, vsa_extend_edist_host): editextend
   (kurtz/extendED.c:78-355) for every seed of a list in host memory, by the
   rules of extend_edist_rules.h, which the kernels of extend_edist.hip read
   too.  No GPU involved; any distance bound the record carries; the seeds
   are dealt out to threads in pieces, the matches come out in the order of
   the seeds.  The query batch is laid out as the reference's Multiseq first,
   one array with a separator between two sequences, wherever its sequences
   lie in querysymbols. */
#include <stdlib.h>
#include <string.h>
#include "vstree_amd.h"
#include "extend_host_common.h"
#include "extend_edist_rules.h"

#define WHO "vsa_extend_edist_host"

typedef struct
{
  const uint8_t *text, *seq2; /* the two Multiseqs */
  uint64_t n, n2;
  const uint64_t *abs2; /* where the query sequences begin in seq2 */
  int self;
  uint64_t leastlength, maxdist, seedlength;
  int bytewise;
  const vsa_selrules *ev;
} Job;

/* vsa_exthost_seed: scratch is the fronts of the two sides */
static int extendseed(const void *job, void *scratch, const vsa_match *m,
                      uint64_t where, vsa_match *out)
{
  const Job *j = (const Job *) job;
  const uint64_t pos2 = j->self ? where : j->abs2[where] + m->querystart;
  uint64_t *lf = (uint64_t *) scratch,
           *rf = lf + vsa_ed_frontwords(j->maxdist);
  vsa_ed_side ls, rs;
  vsa_ed_match best = {0, 0, 0, 0, 0};
  uint32_t hleft, hright;

  vsa_ed_side_init(&ls, j->text, j->n, j->seq2, j->n2, j->self, m->dbstart,
                   pos2, m->length, 1, j->maxdist, j->seedlength);
  vsa_ed_side_init(&rs, j->text, j->n, j->seq2, j->n2, j->self, m->dbstart,
                   pos2, m->length, 0, j->maxdist, j->seedlength);
  hleft = vsa_ed_fronts(&ls, lf, j->bytewise);
  hright = vsa_ed_fronts(&rs, rf, j->bytewise);
  if (!vsa_ed_choose(j->ev, &ls, &rs, j->self, m->dbstart, pos2, m->length,
                     j->leastlength, lf, hleft, rf, hright, &best))
  {
    return 0;
  }
  vsa_ed_record(m, j->self, pos2, &best, out);
  return 1;
}

static void *extendpiece(void *piece)
{
  return vsa_exthost_dopiece(piece, extendseed);
}

int vsa_extend_edist_host(const vsa_sinkparams *layout, const uint8_t *text,
                          const uint8_t *querysymbols, const vsa_match *seeds,
                          uint64_t numofseeds, uint64_t leastlength,
                          uint64_t maxdist, uint64_t seedlength, int threads,
                          vsa_match *matches, uint64_t capacity,
                          uint64_t *numofmatches)
{
  vsa_evalues ev;
  vsa_selrules evrules;
  Job job;
  uint8_t *seq2 = NULL;
  uint64_t *abs2 = NULL;
  double *hequot = NULL;
  const char *scalar = getenv("VSA_EXTEND_EDIST_SCALAR");
  uint64_t i;
  int rc = vsa_exthost_check(WHO, layout, text, querysymbols, seeds,
                             numofseeds, leastlength, maxdist,
                             VSA_EDIST_MAXDISTANCE, matches, capacity,
                             numofmatches);

  if (rc != 0 || numofseeds == 0)
  {
    return rc;
  }
  vsa_evalues_init(&ev, layout->numofchars);
  memset(&evrules, 0, sizeof evrules);
  memset(&job, 0, sizeof job);
  hequot = (double *) malloc((maxdist + 1) * sizeof *hequot);
  if (vsa_evalues_extend(&ev, (int64_t) maxdist) != 0 || hequot == NULL)
  {
    rc = vsa_fail(-101, "out of memory");
    goto done;
  }
  for (i = 0; i <= maxdist; i++)
  {
    hequot[i] = i <= VSA_EVALUES_MAXEDIST ? vsa_evalues_hequot((int64_t) i)
                                          : 0.0;
  }
  if (layout->kind == VSA_SINK_QUERY)
  {
    /* the query Multiseq */
    const uint64_t nq = layout->numofqueries;
    uint64_t total = 0;
    for (i = 0; i < nq; i++)
    {
      total += layout->querylength[i] + (i > 0 ? 1 : 0);
    }
    seq2 = (uint8_t *) malloc(total + 1);
    abs2 = (uint64_t *) malloc((nq + 1) * sizeof *abs2);
    if (seq2 == NULL || abs2 == NULL)
    {
      rc = vsa_fail(-101, "out of memory");
      goto done;
    }
    total = 0;
    for (i = 0; i < nq; i++)
    {
      if (i > 0)
      {
        seq2[total++] = (uint8_t) VSA_SEPARATOR;
      }
      abs2[i] = total;
      if (layout->querylength[i] > 0)
      {
        memcpy(seq2 + total, querysymbols + layout->querystart[i],
               layout->querylength[i]);
      }
      total += layout->querylength[i];
    }
    job.seq2 = seq2;
    job.n2 = total;
    job.abs2 = abs2;
  } else
  {
    job.seq2 = text;
    job.n2 = layout->totallength;
  }
  evrules.table = ev.table;
  evrules.linestart = ev.linestart;
  evrules.hequot = hequot;
  evrules.nlines = (int64_t) maxdist + 1;
  job.text = text;
  job.n = layout->totallength;
  job.self = layout->kind == VSA_SINK_SELF;
  job.leastlength = leastlength;
  job.maxdist = maxdist;
  job.seedlength = vsa_ext_seedlength(leastlength, maxdist, seedlength);
  job.bytewise = scalar != NULL && *scalar != '\0' && *scalar != '0';
  job.ev = &evrules;
  rc = vsa_exthost_extend(WHO, layout, seeds, numofseeds, threads, 64,
                          extendpiece, &job,
                          2 * vsa_ed_frontwords(maxdist) * sizeof(uint64_t),
                          matches, capacity, numofmatches);
done:
  free(hequot);
  free(seq2);
  free(abs2);
  vsa_evalues_free(&ev);
  return rc;
}
