/*
  What the host sides of the two extensions of exact seeds share
  (extend_host.c: -h K, extend_edist_host.c: -e K), stated ONCE: the checks of
  the arguments and of the layout, the test that a seed fits the layout, and
  the runner that deals the seeds out to threads, collects what they could
  not do and copies the matches out in the order of the seeds.  Each file
  keeps its Job, its worker for one seed and what it alone prepares.  Static
  inline functions only, as in host_common.h: no object file and no symbol of
  its own.
*/
#ifndef VSA_EXTEND_HOST_COMMON_H
#define VSA_EXTEND_HOST_COMMON_H
#include <pthread.h>
#include <stdlib.h>
#include <unistd.h>
#include "host_common.h"

/* what an entry refuses before anything is made; cap: the largest distance
   bound its record carries.  *numofmatches is 0 behind the first check. */
static inline int vsa_exthost_check(const char *who,
                                    const vsa_sinkparams *layout,
                                    const uint8_t *text,
                                    const uint8_t *querysymbols,
                                    const vsa_match *seeds,
                                    uint64_t numofseeds, uint64_t leastlength,
                                    uint64_t maxdist, unsigned cap,
                                    const vsa_match *matches,
                                    uint64_t capacity, uint64_t *numofmatches)
{
  if (layout == NULL || text == NULL || numofmatches == NULL ||
      (matches == NULL && capacity > 0))
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  *numofmatches = 0;
  if (vsa_list_check(who, NULL, seeds, numofseeds) != 0)
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
    return vsa_fail(-2, "%s: the seeds of a query layout (VSA_SINK_QUERY, "
                    "with the query symbols) or of a self layout "
                    "(VSA_SINK_SELF) are extended", who);
  }
  if (maxdist == 0 || maxdist > cap || leastlength == 0)
  {
    return vsa_fail(-2, "%s: a least length and a distance bound from 1 to "
                    "%u", who, cap);
  }
  return 0;
}

/* does seed m fit the layout?  *where: its position in the text (a self
   layout) or the number of its query sequence */
static inline int vsa_exthost_fits(const vsa_sinkparams *lay,
                                   const vsa_match *m, uint64_t *where)
{
  const uint64_t n = lay->totallength;

  *where = m->queryseq;
  if (m->length == 0 || m->dbstart > n || m->length > n - m->dbstart)
  {
    return 0;
  }
  if (lay->kind == VSA_SINK_SELF)
  {
    return m->queryseq <= n && m->length <= n - m->queryseq;
  }
  return m->queryseq < lay->numofqueries &&
         m->querystart <= lay->querylength[m->queryseq] &&
         m->length <= lay->querylength[m->queryseq] - m->querystart;
}

/* the worker of a kind for one seed that fits: scratch is the thread's own,
   `where` what vsa_exthost_fits gave; 1 and the match in *out, or 0 (below
   0: out of memory) */
typedef int vsa_exthost_seed(const void *job, void *scratch,
                             const vsa_match *m, uint64_t where,
                             vsa_match *out);

typedef struct
{
  const vsa_sinkparams *layout;
  const vsa_match *seeds;
  const void *job;
  size_t scratchbytes;
  vsa_match *out; /* out[i]: the match of seed i, where keep[i] */
  uint8_t *keep;
} vsa_exthost_run;

typedef struct
{
  const vsa_exthost_run *run;
  uint64_t first, last;
  int64_t misfit; /* the first seed that does not fit the layout, or -1 */
  int nomem;
} vsa_exthost_piece;

/* the seeds of a piece through `seed`.  A kind wraps it into the function a
   thread runs, `static void *f(void *piece) { return vsa_exthost_dopiece(
   piece, itsworker); }`, so that the worker is compiled into the loop. */
static inline void *vsa_exthost_dopiece(void *arg, vsa_exthost_seed *seed)
{
  vsa_exthost_piece *p = (vsa_exthost_piece *) arg;
  const vsa_exthost_run *r = p->run;
  void *scratch = malloc(r->scratchbytes);
  uint64_t i;

  if (scratch == NULL)
  {
    p->nomem = 1;
    return NULL;
  }
  for (i = p->first; i < p->last; i++)
  {
    uint64_t where;

    r->keep[i] = 0;
    if (!vsa_exthost_fits(r->layout, r->seeds + i, &where))
    {
      p->misfit = (int64_t) i;
      break;
    }
    const int kept = seed(r->job, scratch, r->seeds + i, where, r->out + i);
    if (kept < 0) /* the worker found no memory of its own */
    {
      p->nomem = 1;
      break;
    }
    r->keep[i] = (uint8_t) kept;
  }
  free(scratch);
  return NULL;
}

/* numofseeds > 0 seeds through `dopiece` (see vsa_exthost_dopiece) on up to
   256 threads (threads <= 0: as many as there are processors), at least
   `grain` seeds each; a piece whose thread did not start is run by the
   caller.  The matches in the order of the seeds -> matches, *numofmatches;
   -101 without memory, -2 with a seed that does not fit, -3 with more than
   `capacity` matches. */
static inline int vsa_exthost_extend(const char *who,
                                     const vsa_sinkparams *layout,
                                     const vsa_match *seeds,
                                     uint64_t numofseeds, int threads,
                                     uint64_t grain, void *(*dopiece)(void *),
                                     const void *job, size_t scratchbytes,
                                     vsa_match *matches, uint64_t capacity,
                                     uint64_t *numofmatches)
{
  enum { MAXTHREADS = 256 };
  pthread_t tid[MAXTHREADS];
  vsa_exthost_piece piece[MAXTHREADS];
  vsa_exthost_run run;
  uint64_t i, kept = 0;
  int t, nt, started = 0, rc = 0;

  run.layout = layout;
  run.seeds = seeds;
  run.job = job;
  run.scratchbytes = scratchbytes;
  run.out = (vsa_match *) malloc(numofseeds * sizeof *run.out);
  run.keep = (uint8_t *) malloc(numofseeds);
  if (run.out == NULL || run.keep == NULL)
  {
    rc = vsa_fail(-101, "out of memory");
    goto done;
  }
  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  if ((uint64_t) nt > (numofseeds + grain - 1) / grain)
  {
    nt = (int) ((numofseeds + grain - 1) / grain);
  }
  for (t = 0; t < nt; t++)
  {
    piece[t].run = &run;
    piece[t].first = numofseeds * (uint64_t) t / (uint64_t) nt;
    piece[t].last = numofseeds * (uint64_t) (t + 1) / (uint64_t) nt;
    piece[t].misfit = -1;
    piece[t].nomem = 0;
  }
  for (t = 1; t < nt; t++)
  {
    if (pthread_create(tid + t, NULL, dopiece, piece + t) != 0)
    {
      break;
    }
    started = t;
  }
  (void) dopiece(piece);
  for (t = started + 1; t < nt; t++) /* the pieces no thread took */
  {
    (void) dopiece(piece + t);
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
      rc = vsa_list_misfit(who, (uint64_t) piece[t].misfit);
    }
  }
  for (i = 0; i < numofseeds && rc == 0; i++)
  {
    if (run.keep[i])
    {
      if (kept == capacity)
      {
        rc = vsa_fail(-3, "%s: more than %lu matches", who,
                      (unsigned long) capacity);
        break;
      }
      matches[kept++] = run.out[i];
    }
  }
  if (rc == 0)
  {
    *numofmatches = kept;
  }
done:
  free(run.out);
  free(run.keep);
  return rc;
}

#endif
