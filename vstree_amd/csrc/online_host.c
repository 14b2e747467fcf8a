/* Host side of the scan without an index (include/vstree_amd_online.h,
   vsa_findcompletematches_online_host): vmatch -online -complete [remred]
   [-e K | -h K] by the rules of online_rules.h, which the kernels of
   online.hip read too.  No GPU involved; any pattern length, alphabet and
   threshold.  The work is cut by (query, slice of the text) and dealt out to
   threads; an edit scan of a slice starts vsa_online_warmup() symbols to its
   right with a reset column.  remred runs over the merged start positions of
   a query, which come out in the order of the reference. */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "vstree_amd.h"
#include "host_common.h"
#include "online_rules.h"

#define WHO "vsa_findcompletematches_online_host"
#define MINSLICE 64u /* symbols of a slice at least */

typedef struct
{
  uint64_t pos, score;
} Hit;

typedef struct
{
  Hit *h;
  uint64_t n, cap;
} HitList;

typedef struct
{
  const uint8_t *tis, *qsym;
  const uint64_t *qstart, *qlen;
  uint64_t n, nq, distvalue, slices, next;
  int mode, percent, failed;
  HitList *lists; /* [nq * slices] */
} Job;

static int push(HitList *l, uint64_t pos, uint64_t score)
{
  if (l->n == l->cap)
  {
    const uint64_t cap = l->cap ? 2 * l->cap : 16;
    Hit *h = (Hit *) realloc(l->h, cap * sizeof *h);
    if (h == NULL)
    {
      return -1;
    }
    l->h = h;
    l->cap = cap;
  }
  l->h[l->n].pos = pos;
  l->h[l->n].score = score;
  l->n++;
  return 0;
}

/* ---- the column of Myers' algorithm over any number of words -------------- */

typedef struct
{
  uint64_t *eq; /* [256 * words]: the Eq mask of every text symbol */
  uint64_t *pv, *mv, words, m, score;
} Column;

static void column_free(Column *c)
{
  free(c->eq);
  free(c->pv);
  free(c->mv);
  c->eq = c->pv = c->mv = NULL;
}

/* scan != 0: the reversed pattern under the equality of the scan for start
   positions; else the pattern as it is under the equality of longestmatch.c */
static int column_init(Column *c, const uint8_t *pattern, uint64_t m,
                       int scan)
{
  const int raw = vsa_online_rawequal(m);
  uint64_t i;

  c->words = (m + 63) / 64;
  c->m = m;
  c->eq = (uint64_t *) calloc(256 * c->words, sizeof *c->eq);
  c->pv = (uint64_t *) malloc(c->words * sizeof *c->pv);
  c->mv = (uint64_t *) malloc(c->words * sizeof *c->mv);
  if (c->eq == NULL || c->pv == NULL || c->mv == NULL)
  {
    column_free(c);
    return -1;
  }
  for (i = 0; i < m; i++)
  {
    const uint8_t p = pattern[scan ? m - 1 - i : i];
    if (scan ? vsa_online_scanequal(p, p, raw) : vsa_online_longestequal(p, p))
    {
      c->eq[(uint64_t) p * c->words + (i >> 6)] |= 1ull << (i & 63);
    }
  }
  return 0;
}

/* column 0: D[i] = i */
static void column_reset(Column *c)
{
  uint64_t w;

  for (w = 0; w < c->words; w++)
  {
    c->pv[w] = ~0ull;
    c->mv[w] = 0;
  }
  c->score = c->m;
}

/* the next column for text symbol t (no separator); hin = the change of row
   0: 0 if an occurrence may start anywhere, +1 for a global alignment */
static void column_step(Column *c, uint8_t t, int hin)
{
  const uint64_t *eqrow = c->eq + (uint64_t) t * c->words,
                 topbit = 1ull << ((c->m - 1) & 63);
  uint64_t w;

  for (w = 0; w < c->words; w++)
  {
    uint64_t eq = eqrow[w];
    const uint64_t p = c->pv[w], n = c->mv[w], xv = eq | n,
                   top = (w + 1 == c->words) ? topbit : (1ull << 63);
    uint64_t xh, ph, mh;
    int hout;

    if (hin < 0)
    {
      eq |= 1ull;
    }
    xh = (((eq & p) + p) ^ p) | eq;
    ph = n | ~(xh | p);
    mh = p & xh;
    hout = (ph & top) ? 1 : ((mh & top) ? -1 : 0);
    ph <<= 1;
    mh <<= 1;
    if (hin < 0)
    {
      mh |= 1ull;
    } else if (hin > 0)
    {
      ph |= 1ull;
    }
    c->pv[w] = mh | ~(xv | ph);
    c->mv[w] = ph & xv;
    hin = hout;
  }
  c->score = (uint64_t) ((int64_t) c->score + hin);
}

/* ---- one (query, slice) --------------------------------------------------- */

/* the start positions in [a, b), descending */
static int scan_edist(const Job *j, uint64_t q, uint64_t a, uint64_t b,
                      HitList *out)
{
  const uint64_t m = j->qlen[q],
                 k = vsa_online_threshold(m, j->distvalue, j->percent),
                 warm = vsa_online_warmup(m, k);
  uint64_t t = (j->n - b > warm) ? b + warm : j->n;
  Column col;
  int rc = 0;

  if (m == 0 || column_init(&col, j->qsym + j->qstart[q], m, 1) != 0)
  {
    return m == 0 ? 0 : -1;
  }
  column_reset(&col);
  while (t-- > a && rc == 0)
  {
    const uint8_t c = j->tis[t];
    if (c == (uint8_t) VSA_SEPARATOR)
    {
      column_reset(&col);
    } else
    {
      column_step(&col, c, 0);
      if (t < b && vsa_online_isstart(col.score, k))
      {
        rc = push(out, t, col.score);
      }
    }
  }
  column_free(&col);
  return rc;
}

/* the windows that start in [a, b): ascending for the exact scan, descending
   for Hamming distance */
static int scan_windows(const Job *j, uint64_t q, uint64_t a, uint64_t b,
                        HitList *out)
{
  const uint64_t m = j->qlen[q],
                 k = j->mode == VSA_ONLINE_EXACT
                         ? 0
                         : vsa_online_threshold(m, j->distvalue, j->percent);
  const uint8_t *pattern = j->qsym + j->qstart[q];
  uint64_t i, cnt;

  if (m == 0 || m > j->n)
  {
    return 0;
  }
  if (b > j->n - m + 1)
  {
    b = j->n - m + 1;
  }
  cnt = b > a ? b - a : 0;
  for (i = 0; i < cnt; i++)
  {
    const uint64_t t = j->mode == VSA_ONLINE_EXACT ? a + i : b - 1 - i;
    uint64_t o, mm = 0;
    int barred = 0;

    for (o = 0; o < m && !barred && mm <= k; o += 8)
    {
      const uint32_t c = m - o < 8 ? (uint32_t) (m - o) : 8;
      uint64_t tw = 0, pw = 0;
      memcpy(&tw, j->tis + t + o, c);
      memcpy(&pw, pattern + o, c);
      mm += vsa_online_word(tw, pw, c, j->mode, &barred);
    }
    if (!barred && mm <= k && push(out, t, mm) != 0)
    {
      return -1;
    }
  }
  return 0;
}

static void *worker(void *arg)
{
  Job *j = (Job *) arg;
  const uint64_t items = j->nq * j->slices;

  for (;;)
  {
    const uint64_t it = __atomic_fetch_add(&j->next, 1, __ATOMIC_RELAXED);
    uint64_t q, s, a, b;
    int rc;

    if (it >= items)
    {
      break;
    }
    q = it / j->slices;
    s = it % j->slices;
    a = (uint64_t) (((unsigned __int128) j->n * s) / j->slices);
    b = (uint64_t) (((unsigned __int128) j->n * (s + 1)) / j->slices);
    rc = j->mode == VSA_ONLINE_EDIST
             ? scan_edist(j, q, a, b, j->lists + it)
             : scan_windows(j, q, a, b, j->lists + it);
    if (rc != 0)
    {
      __atomic_store_n(&j->failed, 1, __ATOMIC_RELAXED);
    }
  }
  return NULL;
}

/* ---- the records of one query --------------------------------------------- */

typedef struct
{
  vsa_match *out;
  uint64_t n, capacity;
} Sink;

static int emit(Sink *s, uint64_t length, uint64_t dbstart, uint64_t queryseq,
                uint64_t distance)
{
  if (s->n == s->capacity)
  {
    return vsa_fail(-3, WHO ": more than %lu matches",
                    (unsigned long) s->capacity);
  }
  s->out[s->n].length = length;
  s->out[s->n].dbstart = dbstart;
  s->out[s->n].queryseq = queryseq;
  s->out[s->n].querystart = distance;
  s->n++;
  return 0;
}

/* edistprocessstartpos */
static int startpos(const Job *j, Column *col, uint64_t k, uint64_t start,
                    uint64_t queryseq, Sink *s)
{
  const uint64_t vlen = vsa_online_maxlength(col->m, k, j->n, start);
  uint64_t i, bestlen = 0, bestdist = col->m;

  column_reset(col);
  for (i = 0; i < vlen; i++)
  {
    const uint8_t c = j->tis[start + i];
    if (c == (uint8_t) VSA_SEPARATOR)
    {
      break;
    }
    column_step(col, c, 1);
    if (bestdist >= col->score) /* UPDATELENGTHANDSCORE, longestmatch.c:6-11 */
    {
      bestlen = i + 1;
      bestdist = col->score;
    }
  }
  return emit(s, bestlen, start, queryseq, bestdist);
}

static int query_records(const Job *j, uint64_t q, uint64_t queryseq,
                         int removeredundant, Sink *s)
{
  const uint64_t m = j->qlen[q];
  uint64_t si, i;
  int rc = 0;

  if (j->mode != VSA_ONLINE_EDIST)
  {
    for (si = 0; si < j->slices && rc == 0; si++)
    {
      const HitList *l = j->lists + q * j->slices +
                         (j->mode == VSA_ONLINE_EXACT ? si
                                                      : j->slices - 1 - si);
      for (i = 0; i < l->n && rc == 0; i++)
      {
        rc = emit(s, m, l->h[i].pos, queryseq, l->h[i].score);
      }
    }
    return rc;
  }
  {
    const uint64_t k = vsa_online_threshold(m, j->distvalue, j->percent);
    vsa_online_remred state;
    Column col;
    uint64_t flush, any = 0;

    for (si = 0; si < j->slices; si++)
    {
      any += j->lists[q * j->slices + si].n;
    }
    if (any == 0)
    {
      return 0;
    }
    if (column_init(&col, j->qsym + j->qstart[q], m, 0) != 0)
    {
      return vsa_fail(-101, "out of memory");
    }
    vsa_online_remred_init(&state);
    for (si = j->slices; si-- > 0 && rc == 0;)
    {
      const HitList *l = j->lists + q * j->slices + si;
      for (i = 0; i < l->n && rc == 0; i++)
      {
        if (!removeredundant)
        {
          rc = startpos(j, &col, k, l->h[i].pos, queryseq, s);
        } else if (vsa_online_remred_step(&state, l->h[i].pos, l->h[i].score,
                                          &flush))
        {
          rc = startpos(j, &col, k, flush, queryseq, s);
        }
      }
    }
    if (rc == 0 && removeredundant && vsa_online_remred_end(&state, &flush))
    {
      rc = startpos(j, &col, k, flush, queryseq, s);
    }
    column_free(&col);
  }
  return rc;
}

int vsa_findcompletematches_online_host(
    const uint8_t *tis, uint64_t totallength, const uint8_t *querysymbols,
    const uint64_t *querystart, const uint64_t *querylength,
    uint64_t numofqueries, uint64_t seqoffset, int mode, uint64_t distvalue,
    int percent, int removeredundant, int threads, vsa_match *matches,
    uint64_t capacity, uint64_t *numofmatches)
{
  enum { MAXTHREADS = 256 };
  pthread_t tid[MAXTHREADS];
  Job job;
  Sink sink;
  uint64_t q, i;
  int nt, t, started, rc = 0;

  if (numofmatches == NULL || (tis == NULL && totallength > 0) ||
      (matches == NULL && capacity > 0) ||
      (numofqueries > 0 &&
       (querysymbols == NULL || querystart == NULL || querylength == NULL)))
  {
    return vsa_fail(-1, WHO ": NULL argument");
  }
  *numofmatches = 0;
  if (mode < VSA_ONLINE_EXACT || mode > VSA_ONLINE_HAMMING)
  {
    return vsa_fail(-2, WHO ": mode %d: expected 0 (exact), 1 (-e) or 2 (-h)",
                    mode);
  }
  if (removeredundant && mode != VSA_ONLINE_EDIST)
  {
    /* Vmatch/parsevm.c:1448 */
    return vsa_fail(-2, "argument \"remred\" of option -complete requires "
                    "options -e or -h");
  }
  if (percent == 2)
  {
    return vsa_fail(VSA_NOT_COVERED, WHO ": -online with Kb (best of) is not "
                    "covered");
  }
  if (numofqueries == 0 || totallength == 0)
  {
    return 0;
  }
  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  memset(&job, 0, sizeof job);
  job.tis = tis;
  job.n = totallength;
  job.qsym = querysymbols;
  job.qstart = querystart;
  job.qlen = querylength;
  job.nq = numofqueries;
  job.mode = mode;
  job.distvalue = distvalue;
  job.percent = percent != 0;
  /* about two items per thread, no slice below MINSLICE symbols */
  job.slices = nt == 1 ? 1 : (2 * (uint64_t) nt + numofqueries - 1) /
                                 numofqueries;
  if (job.slices > totallength / MINSLICE)
  {
    job.slices = totallength / MINSLICE;
  }
  if (job.slices < 1)
  {
    job.slices = 1;
  }
  job.lists = (HitList *) calloc(numofqueries * job.slices,
                                 sizeof *job.lists);
  if (job.lists == NULL)
  {
    return vsa_fail(-101, "out of memory");
  }
  started = 0;
  for (t = 1; t < nt; t++)
  {
    if (pthread_create(tid + t, NULL, worker, &job) != 0)
    {
      break;
    }
    started = t;
  }
  (void) worker(&job);
  for (t = 1; t <= started; t++)
  {
    pthread_join(tid[t], NULL);
  }
  if (job.failed)
  {
    rc = vsa_fail(-101, "out of memory");
  }
  sink.out = matches;
  sink.n = 0;
  sink.capacity = capacity;
  for (q = 0; q < numofqueries && rc == 0; q++)
  {
    rc = query_records(&job, q, q + seqoffset, removeredundant, &sink);
  }
  for (i = 0; i < numofqueries * job.slices; i++)
  {
    free(job.lists[i].h);
  }
  free(job.lists);
  *numofmatches = rc == 0 ? sink.n : 0;
  return rc;
}
