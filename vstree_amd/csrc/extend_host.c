/* Host side of the Hamming extension of exact seeds (include/vstree_amd.h,
   vsa_extend_hamming_host): hammingextend (kurtz/extendHD.c:166-374) for
   every seed of a list in host memory, by the rules of extend_rules.h, which
   the kernels of extend.hip read too.  No GPU involved; any distance bound;
   the seeds are dealt out to threads in pieces, the matches come out in the
   order of the seeds. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "vstree_amd.h"
#include "host_common.h"
#include "extend_rules.h"

#define WHO "vsa_extend_hamming_host"

typedef struct
{
  const vsa_sinkparams *layout;
  const uint8_t *text, *querysymbols;
  const vsa_match *seeds;
  uint64_t leastlength, maxdist, seedlength;
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

/* one side of seed: its look table, and the mismatches it offers */
static uint32_t scanside(const Job *j, int left, const vsa_ext_view *v1,
                         uint64_t pos1, const vsa_ext_view *v2, uint64_t pos2,
                         uint64_t length, uint64_t *look)
{
  vsa_ext_scan s;
  vsa_ext_plan plan;
  uint32_t h = 0;
  uint64_t t0;

  vsa_ext_begin(&s, look, 1, (uint32_t) j->maxdist, j->seedlength, left);
  if (vsa_ext_prepare(&s, v1, pos1, v2, pos2, length, &plan, &h) ==
      VSA_EXT_FIXED)
  {
    return h;
  }
  for (t0 = 0; t0 < plan.nsym; t0 += 8)
  {
    uint32_t sep;
    const uint64_t a = vsa_ext_word(plan.p1, left, t0, plan.nsym - t0),
                   b = vsa_ext_word(plan.p2, left, t0, plan.nsym - t0);
    const uint32_t marks = vsa_ext_marks8(a, b, &sep);

    if (vsa_ext_events(&s, &plan, t0, marks, sep))
    {
      return vsa_ext_end(&s);
    }
  }
  (void) vsa_ext_finish(&s, &plan);
  return vsa_ext_end(&s);
}

static void *extendpiece(void *arg)
{
  Piece *p = (Piece *) arg;
  const Job *j = p->job;
  const vsa_sinkparams *lay = j->layout;
  const int self = lay->kind == VSA_SINK_SELF;
  const uint64_t n = lay->totallength;
  const vsa_ext_view text = {j->text, n, 1, 1};
  uint64_t *look = (uint64_t *) malloc(2 * (j->maxdist + 2) * sizeof *look);
  uint64_t *lookright = look + j->maxdist + 2, i;

  if (look == NULL)
  {
    p->nomem = 1;
    return NULL;
  }
  for (i = p->first; i < p->last; i++)
  {
    const vsa_match *m = j->seeds + i;
    vsa_ext_view v2 = text;
    uint64_t pos2 = m->queryseq, shift = 0, outlength = 0, dist = 0;
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
      v2.p = j->querysymbols + lay->querystart[q];
      v2.len = lay->querylength[q];
      v2.atstart = q == 0;
      v2.atend = q + 1 == lay->numofqueries;
      pos2 = m->querystart;
    }
    hleft = scanside(j, 1, &text, m->dbstart, &v2, pos2, m->length, look);
    hright = scanside(j, 0, &text, m->dbstart, &v2, pos2, m->length,
                      lookright);
    if (vsa_ext_choose(j->ev, m->length, j->leastlength, j->maxdist, look,
                       hleft, lookright, hright, 1, &shift, &outlength,
                       &dist))
    {
      vsa_match *o = j->out + i;
      o->length = VSA_HAMMING_PACK(outlength, dist);
      o->dbstart = m->dbstart - shift;
      o->queryseq = self ? m->queryseq - shift : m->queryseq;
      o->querystart = self ? 0 : m->querystart - shift;
      j->keep[i] = 1;
    }
  }
  free(look);
  return NULL;
}

int vsa_extend_hamming_host(const vsa_sinkparams *layout, const uint8_t *text,
                            const uint8_t *querysymbols,
                            const vsa_match *seeds, uint64_t numofseeds,
                            uint64_t leastlength, uint64_t maxdist,
                            uint64_t seedlength, int threads,
                            vsa_match *matches, uint64_t capacity,
                            uint64_t *numofmatches)
{
  enum { MAXTHREADS = 256 };
  pthread_t tid[MAXTHREADS];
  Piece piece[MAXTHREADS];
  vsa_evalues ev;
  vsa_selrules evrules;
  Job job;
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
  if (maxdist == 0 || maxdist > VSA_HAMMING_MAXDISTANCE || leastlength == 0)
  {
    return vsa_fail(-2, WHO ": a least length and a distance bound from 1 "
                    "to %u", (unsigned) VSA_HAMMING_MAXDISTANCE);
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
  if (vsa_evalues_extend(&ev, (int64_t) maxdist) != 0 || job.out == NULL ||
      job.keep == NULL)
  {
    rc = vsa_fail(-101, "out of memory");
    goto done;
  }
  evrules.table = ev.table;
  evrules.linestart = ev.linestart;
  evrules.nlines = (int64_t) maxdist + 1;
  job.layout = layout;
  job.text = text;
  job.querysymbols = querysymbols;
  job.seeds = seeds;
  job.leastlength = leastlength;
  job.maxdist = maxdist;
  job.seedlength = vsa_ext_seedlength(leastlength, maxdist, seedlength);
  job.ev = &evrules;
  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  if ((uint64_t) nt > (numofseeds + 1023) / 1024)
  {
    nt = (int) ((numofseeds + 1023) / 1024);
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
  vsa_evalues_free(&ev);
  return rc;
}
