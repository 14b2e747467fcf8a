/* Host side of the X-drop extension of exact seeds
   (include/vstree_amd_xdrop.h, vsa_extend_xdrop_host): xdropseedextend
   (Vmengine/xdropext.c:39-221) for every seed of a list in host memory, by
   the rules of extend_xdrop_rules.h, which the kernels of extend_xdrop.hip
   read too.  No GPU involved; any X the reference takes and any band; the
   seeds are dealt out to threads in pieces, the matches come out in the
   order of the seeds.  The query batch is laid out as the reference's
   Multiseq first, as for the edit-distance extension. */
#include <stdlib.h>
#include <string.h>
#include "vstree_amd.h"
#include "extend_host_common.h"
#include "extend_xdrop_rules.h"
#include "extend_xdrop_host.h"

#define WHO "vsa_extend_xdrop_host"

/* the rows of a generation a thread keeps; a wider band gets rows of its
   own for that side */
#define ROWCAP 512
#define ROWBYTES ((2 * ROWCAP + VSA_XD_RING) * sizeof(int64_t))

typedef struct
{
  const uint8_t *text, *seq2; /* the two Multiseqs */
  uint64_t n, n2;
  const uint64_t *abs2; /* where the query sequences begin in seq2 */
  int self, hamming, bytewise;
  uint64_t leastlength, xdrop, seedlength;
} Job;

/* one side by the Hamming scan; VSA_XD_REJECT: no match for this seed */
static int hammingside(const Job *j, int left, uint64_t pos1, uint64_t pos2,
                       uint64_t length, vsa_xd_best *best)
{
  const vsa_ext_view v1 = {j->text, j->n, 1, 1}, v2 = {j->seq2, j->n2, 1, 1};
  vsa_xd_plan plan;
  vsa_xd_scan s;
  uint64_t t0;
  int rc = VSA_XD_ON;

  vsa_xd_prepare(&v1, pos1, &v2, pos2, length, left, &plan);
  vsa_xd_begin(&s, j->xdrop, j->seedlength, left);
  for (t0 = 0; rc == VSA_XD_ON && t0 < plan.nsym; t0 += j->bytewise ? 1 : 8)
  {
    const uint64_t valid = j->bytewise ? 1 : plan.nsym - t0;
    uint32_t sep;
    const uint32_t marks =
        vsa_ext_marks8(vsa_ext_word(plan.p1, left, t0, valid),
                       vsa_ext_word(plan.p2, left, t0, valid), &sep);

    rc = vsa_xd_events(&s, &plan, t0, marks, sep);
    if (rc == VSA_XD_ON)
    {
      rc = vsa_xd_upto(&s, &plan, t0 + (j->bytewise ? 1 : 8));
    }
  }
  if (rc == VSA_XD_ON)
  {
    rc = vsa_xd_finishside(&s, &plan);
  }
  vsa_xd_scanbest(&s, best);
  return rc;
}

/* one side by the generations; -1 without memory */
static int editside(const Job *j, int64_t *rows, int left, uint64_t pos1,
                    uint64_t pos2, uint64_t length, vsa_xd_best *best)
{
  int64_t *wide = NULL, *g = rows, cap = ROWCAP;
  int rc = 0;

  for (;;)
  {
    vsa_xd_arrays a;

    best->ivalue = best->jvalue = best->score = 0;
    if (!vsa_xd_arrays_init(&a, j->text, j->n, j->seq2, j->n2, pos1, pos2,
                            length, left) ||
        !vsa_xd_editside(&a, (int64_t) j->xdrop, g, g + cap, cap, g + 2 * cap,
                         j->bytewise, best))
    {
      break;
    }
    /* a generation wider than the rows: once more from the start */
    cap *= 4;
    free(wide);
    wide = (int64_t *) malloc(((size_t) 2 * (size_t) cap + VSA_XD_RING) *
                              sizeof *wide);
    if (wide == NULL)
    {
      rc = -1;
      break;
    }
    g = wide;
  }
  free(wide);
  return rc;
}

/* seed m, at pos2 of the second Multiseq; rows: two rows and the ring of T
   values.  1 and *out, 0, or -1 without memory */
static int extendat(const Job *j, int64_t *rows, const vsa_match *m,
                    uint64_t pos2, vsa_match *out)
{
  vsa_xd_best l, r;
  vsa_xd_match x;

  if (j->hamming)
  {
    if (hammingside(j, 1, m->dbstart, pos2, m->length, &l) == VSA_XD_REJECT)
    {
      return 0;
    }
    (void) hammingside(j, 0, m->dbstart, pos2, m->length, &r);
  } else if (editside(j, rows, 1, m->dbstart, pos2, m->length, &l) != 0 ||
             editside(j, rows, 0, m->dbstart, pos2, m->length, &r) != 0)
  {
    return -1;
  }
  if (!vsa_xd_finish(j->text, j->seq2, j->self, j->hamming, m->dbstart, pos2,
                     m->length, &l, &r, j->leastlength, &x))
  {
    return 0;
  }
  vsa_xd_record(m, j->self, pos2, &x, out);
  return 1;
}

/* vsa_exthost_seed */
static int extendseed(const void *job, void *scratch, const vsa_match *m,
                      uint64_t where, vsa_match *out)
{
  const Job *j = (const Job *) job;

  return extendat(j, (int64_t *) scratch, m,
                  j->self ? where : j->abs2[where] + m->querystart, out);
}

/* the seeds first .. last - 1 of a call of vsa_xd_host_seeds */
typedef struct
{
  const Job *job;
  const vsa_match *seeds;
  const uint64_t *pos2;
  vsa_match *out;
  uint8_t *keep;
  uint64_t first, last;
  int nomem;
} Part;

static void *dopart(void *arg)
{
  Part *p = (Part *) arg;
  int64_t *rows = (int64_t *) malloc(ROWBYTES);
  uint64_t i;

  p->nomem = rows == NULL;
  for (i = p->first; i < p->last && !p->nomem; i++)
  {
    const int kept = extendat(p->job, rows, p->seeds + i, p->pos2[i],
                              p->out + i);
    p->keep[i] = (uint8_t) (kept > 0);
    p->nomem = kept < 0;
  }
  free(rows);
  return NULL;
}

int vsa_xd_host_seeds(const uint8_t *seq1, uint64_t n1, const uint8_t *seq2,
                      uint64_t n2, int self, int hamming,
                      const vsa_match *seeds, const uint64_t *pos2,
                      uint64_t numofseeds, uint64_t leastlength,
                      uint64_t xdrop, uint64_t seedlength, int threads,
                      vsa_match *out, uint8_t *keep)
{
  enum { MAXTHREADS = 64 };
  pthread_t tid[MAXTHREADS];
  Part part[MAXTHREADS];
  Job job;
  int t, nt, started = 0, nomem = 0;

  memset(&job, 0, sizeof job);
  job.text = seq1;
  job.n = n1;
  job.seq2 = seq2;
  job.n2 = n2;
  job.self = self;
  job.hamming = hamming;
  job.leastlength = leastlength;
  job.xdrop = xdrop;
  job.seedlength = seedlength;
  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  if ((uint64_t) nt > numofseeds)
  {
    nt = numofseeds > 0 ? (int) numofseeds : 1;
  }
  for (t = 0; t < nt; t++)
  {
    part[t].job = &job;
    part[t].seeds = seeds;
    part[t].pos2 = pos2;
    part[t].out = out;
    part[t].keep = keep;
    part[t].first = numofseeds * (uint64_t) t / (uint64_t) nt;
    part[t].last = numofseeds * (uint64_t) (t + 1) / (uint64_t) nt;
    part[t].nomem = 0;
  }
  for (t = 1; t < nt; t++)
  {
    if (pthread_create(tid + t, NULL, dopart, part + t) != 0)
    {
      break;
    }
    started = t;
  }
  (void) dopart(part);
  for (t = started + 1; t < nt; t++) /* the parts no thread took */
  {
    (void) dopart(part + t);
  }
  for (t = 1; t <= started; t++)
  {
    (void) pthread_join(tid[t], NULL);
  }
  for (t = 0; t < nt; t++)
  {
    nomem |= part[t].nomem;
  }
  return nomem ? vsa_fail(-101, "out of memory") : 0;
}

static void *extendpiece(void *piece)
{
  return vsa_exthost_dopiece(piece, extendseed);
}

int vsa_extend_xdrop_host(const vsa_sinkparams *layout, const uint8_t *text,
                          const uint8_t *querysymbols, const vsa_match *seeds,
                          uint64_t numofseeds, uint64_t leastlength,
                          uint64_t xdrop, int hamming, uint64_t seedlength,
                          int threads, vsa_match *matches, uint64_t capacity,
                          uint64_t *numofmatches)
{
  Job job;
  uint8_t *seq2 = NULL;
  uint64_t *abs2 = NULL;
  const char *scalar = getenv("VSA_EXTEND_XDROP_SCALAR");
  uint64_t i;
  /* (the bound of X has words of its own below: any X passes here) */
  int rc = vsa_exthost_check(WHO, layout, text, querysymbols, seeds,
                             numofseeds, leastlength,
                             xdrop > VSA_XDROP_MAXDROP ? 1 : xdrop,
                             VSA_XDROP_MAXDROP, matches, capacity,
                             numofmatches);

  if (rc != 0)
  {
    return rc;
  }
  if (xdrop > VSA_XDROP_MAXDROP)
  {
    return vsa_fail(-2, "%s: X = %lu: the reference takes 1 to %u (FLAGXDROP, "
                    "Vmatch/parsevm.c)", WHO, (unsigned long) xdrop,
                    VSA_XDROP_MAXDROP);
  }
  /* what the record cannot carry */
  rc = layout->totallength >= 0xFFFFFFF0ull;
  for (i = 0; rc == 0 && layout->kind == VSA_SINK_QUERY &&
              i < layout->numofqueries; i++)
  {
    rc = layout->querylength[i] >= 0xFFFFFFF0ull;
  }
  if (rc != 0)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: texts and query sequences below "
                    "2^32 - 16 symbols are covered", WHO);
  }
  if (numofseeds == 0)
  {
    return 0;
  }
  memset(&job, 0, sizeof job);
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
  job.text = text;
  job.n = layout->totallength;
  job.self = layout->kind == VSA_SINK_SELF;
  job.hamming = hamming != 0;
  job.bytewise = scalar != NULL && *scalar != '\0' && *scalar != '0';
  job.leastlength = leastlength;
  job.xdrop = xdrop;
  job.seedlength = vsa_xd_seedlength(seedlength);
  rc = vsa_exthost_extend(WHO, layout, seeds, numofseeds, threads, 64,
                          extendpiece, &job,
                          ROWBYTES,
                          matches, capacity, numofmatches);
done:
  free(seq2);
  free(abs2);
  return rc;
}
