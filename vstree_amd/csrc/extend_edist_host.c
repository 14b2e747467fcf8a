/* Host side of the edit-distance extension of exact seeds
   (include/vstree_amd_edist.h, vsa_extend_edist_host): editextend
   (kurtz/extendED.c:78-355) for every seed of a list in host memory, by the
   rules of extend_edist_rules.h, which the kernels of extend_edist.hip read
   too.  No GPU involved; any distance bound the record carries; the seeds
   are dealt out to threads in pieces, the matches come out in the order of
   the seeds.  The query batch is laid out as the reference's Multiseq first,
   one array with a separator between two sequences, wherever its sequences
   lie in querysymbols. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "vstree_amd.h"
#include "host_common.h"
#include "extend_edist_rules.h"

#define WHO "vsa_extend_edist_host"

typedef struct
{
  const vsa_sinkparams *layout;
  const uint8_t *text, *seq2; /* the two Multiseqs */
  uint64_t n2;
  const uint64_t *abs2; /* where the query sequences begin in seq2 */
  const vsa_match *seeds;
  uint64_t leastlength, maxdist, seedlength;
  int bytewise;
  const vsa_selrules *ev;
  vsa_match *out; /* out[i]: the match of seed i, where keep[i] */
  uint8_t *keep;
} Job;

typedef struct
{
  const Job *job;
  uint64_t first, last;
  int64_t misfit; /* the first seed that does not fit the layout, or -1 */
  int nomem;
} Piece;

static void *extendpiece(void *arg)
{
  Piece *p = (Piece *) arg;
  const Job *j = p->job;
  const vsa_sinkparams *lay = j->layout;
  const int self = lay->kind == VSA_SINK_SELF;
  const uint64_t n = lay->totallength, words = vsa_ed_frontwords(j->maxdist);
  uint64_t *lf = (uint64_t *) malloc(2 * words * sizeof *lf);
  uint64_t *rf = lf + words, i;

  if (lf == NULL)
  {
    p->nomem = 1;
    return NULL;
  }
  for (i = p->first; i < p->last; i++)
  {
    const vsa_match *m = j->seeds + i;
    uint64_t pos2 = m->queryseq;
    vsa_ed_side ls, rs;
    vsa_ed_match best = {0, 0, 0, 0, 0};
    uint32_t hleft, hright;

    j->keep[i] = 0;
    if (m->length == 0 || m->dbstart > n || m->length > n - m->dbstart)
    {
      p->misfit = (int64_t) i;
      break;
    }
    if (self)
    {
      if (pos2 > n || m->length > n - pos2)
      {
        p->misfit = (int64_t) i;
        break;
      }
    } else
    {
      const uint64_t q = m->queryseq;
      if (q >= lay->numofqueries || m->querystart > lay->querylength[q] ||
          m->length > lay->querylength[q] - m->querystart)
      {
        p->misfit = (int64_t) i;
        break;
      }
      pos2 = j->abs2[q] + m->querystart;
    }
    vsa_ed_side_init(&ls, j->text, n, j->seq2, j->n2, self, m->dbstart, pos2,
                     m->length, 1, j->maxdist, j->seedlength);
    vsa_ed_side_init(&rs, j->text, n, j->seq2, j->n2, self, m->dbstart, pos2,
                     m->length, 0, j->maxdist, j->seedlength);
    hleft = vsa_ed_fronts(&ls, lf, j->bytewise);
    hright = vsa_ed_fronts(&rs, rf, j->bytewise);
    if (vsa_ed_choose(j->ev, &ls, &rs, self, m->dbstart, pos2, m->length,
                      j->leastlength, lf, hleft, rf, hright, &best))
    {
      vsa_ed_record(m, self, pos2, &best, j->out + i);
      j->keep[i] = 1;
    }
  }
  free(lf);
  return NULL;
}

int vsa_extend_edist_host(const vsa_sinkparams *layout, const uint8_t *text,
                          const uint8_t *querysymbols, const vsa_match *seeds,
                          uint64_t numofseeds, uint64_t leastlength,
                          uint64_t maxdist, uint64_t seedlength, int threads,
                          vsa_match *matches, uint64_t capacity,
                          uint64_t *numofmatches)
{
  enum { MAXTHREADS = 256 };
  pthread_t tid[MAXTHREADS];
  Piece piece[MAXTHREADS];
  vsa_evalues ev;
  vsa_selrules evrules;
  Job job;
  uint8_t *seq2 = NULL;
  uint64_t *abs2 = NULL;
  double *hequot = NULL;
  const char *scalar = getenv("VSA_EXTEND_EDIST_SCALAR");
  uint64_t i, kept = 0;
  int t, nt, started = 0, rc = 0;

  if (layout == NULL || text == NULL || numofmatches == NULL ||
      (matches == NULL && capacity > 0))
  {
    return vsa_fail(-1, WHO ": NULL argument");
  }
  *numofmatches = 0;
  if (vsa_list_check(WHO, NULL, seeds, numofseeds) != 0)
  {
    return -1;
  }
  if ((layout->kind != VSA_SINK_QUERY && layout->kind != VSA_SINK_SELF) ||
      layout->totallength == 0 || layout->numofchars < 2 ||
      (layout->kind == VSA_SINK_QUERY &&
       (querysymbols == NULL ||
        (layout->numofqueries > 0 &&
         (layout->querystart == NULL || layout->querylength == NULL)))))
  {
    return vsa_fail(-2, WHO ": the seeds of a query layout "
                    "(VSA_SINK_QUERY, with the query symbols) or of a self "
                    "layout (VSA_SINK_SELF) are extended");
  }
  if (maxdist == 0 || maxdist > VSA_EDIST_MAXDISTANCE || leastlength == 0)
  {
    return vsa_fail(-2, WHO ": a least length and a distance bound from 1 "
                    "to %u", (unsigned) VSA_EDIST_MAXDISTANCE);
  }
  if (numofseeds == 0)
  {
    return 0;
  }
  vsa_evalues_init(&ev, layout->numofchars);
  memset(&evrules, 0, sizeof evrules);
  memset(&job, 0, sizeof job);
  job.out = (vsa_match *) malloc(numofseeds * sizeof *job.out);
  job.keep = (uint8_t *) malloc(numofseeds);
  hequot = (double *) malloc((maxdist + 1) * sizeof *hequot);
  if (vsa_evalues_extend(&ev, (int64_t) maxdist) != 0 || job.out == NULL ||
      job.keep == NULL || hequot == NULL)
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
  job.layout = layout;
  job.text = text;
  job.seeds = seeds;
  job.leastlength = leastlength;
  job.maxdist = maxdist;
  job.seedlength = vsa_ext_seedlength(leastlength, maxdist, seedlength);
  job.bytewise = scalar != NULL && *scalar != '\0' && *scalar != '0';
  job.ev = &evrules;
  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  if ((uint64_t) nt > (numofseeds + 63) / 64)
  {
    nt = (int) ((numofseeds + 63) / 64);
  }
  for (t = 0; t < nt; t++)
  {
    piece[t].job = &job;
    piece[t].first = numofseeds * (uint64_t) t / (uint64_t) nt;
    piece[t].last = numofseeds * (uint64_t) (t + 1) / (uint64_t) nt;
    piece[t].misfit = -1;
    piece[t].nomem = 0;
  }
  for (t = 1; t < nt; t++)
  {
    if (pthread_create(tid + t, NULL, extendpiece, piece + t) != 0)
    {
      break;
    }
    started = t;
  }
  (void) extendpiece(piece);
  for (t = started + 1; t < nt; t++) /* the pieces no thread took */
  {
    (void) extendpiece(piece + t);
  }
  for (t = 1; t <= started; t++)
  {
    (void) pthread_join(tid[t], NULL);
  }
  for (t = 0; t < nt && rc == 0; t++)
  {
    if (piece[t].nomem)
    {
      rc = vsa_fail(-101, "out of memory");
    } else if (piece[t].misfit >= 0)
    {
      rc = vsa_list_misfit(WHO, (uint64_t) piece[t].misfit);
    }
  }
  for (i = 0; i < numofseeds && rc == 0; i++)
  {
    if (job.keep[i])
    {
      if (kept == capacity)
      {
        rc = vsa_fail(-3, WHO ": more than %lu matches",
                      (unsigned long) capacity);
        break;
      }
      matches[kept++] = job.out[i];
    }
  }
  if (rc == 0)
  {
    *numofmatches = kept;
  }
done:
  free(job.out);
  free(job.keep);
  free(hequot);
  free(seq2);
  free(abs2);
  vsa_evalues_free(&ev);
  return rc;
}
