/*
  vmatch -s on the host: the edit scripts of a match list by the rules of
  align_rules.h (vsa_align_host), and the text showalignment prints for
  scripts wherever they were made (vsa_align_format, vsa_align_write;
  kurtz/showalign.c: fillthelines 664-862, showeditopline 1706-1812,
  formatseqwithgaps 1582-1638, formatalignment 1886-2048, with the flags of
  MAKESAFLAG(True, False, selfcomparison)).  The records are dealt out to
  threads in pieces; the scripts and the text come out in record order.
*/
#include <ctype.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "vstree_amd.h"
#include "host_common.h"
#include "align_rules.h"
#include "sink_internal.h"

#define MAXTHREADS 64
#define GAPSYMBOL ((uint8_t) (VSA_SEPARATOR - 3)) /* ABSTRACTGAPSYMBOL */
#define NUMWIDTH 12                               /* showalign.c:600    */
#define DEFAULTLINEWIDTH 60                       /* multidef.h:110     */

/* ---- pieces of a list on threads ------------------------------------------ */

typedef struct
{
  const void *job;
  uint64_t first, last;
  int rc;          /* 0, or the code of the first failure        */
  uint64_t record; /* ... and the record it happened at          */
  void *out;       /* what the worker made of the piece          */
  uint64_t outlen;
} Piece;

/* n records through `work` on up to `threads` threads, at least `grain`
   records each; *npieces pieces in order */
static void runpieces(void *(*work)(void *), const void *job, uint64_t n,
                      int threads, uint64_t grain, Piece *piece, int *npieces)
{
  pthread_t tid[MAXTHREADS];
  int t, nt, started = 0;

  nt = threads > 0 ? threads : (int) sysconf(_SC_NPROCESSORS_ONLN);
  nt = nt < 1 ? 1 : nt > MAXTHREADS ? MAXTHREADS : nt;
  if ((uint64_t) nt > (n + grain - 1) / grain)
  {
    nt = (int) ((n + grain - 1) / grain);
  }
  nt = nt < 1 ? 1 : nt;
  for (t = 0; t < nt; t++)
  {
    memset(piece + t, 0, sizeof *piece);
    piece[t].job = job;
    piece[t].first = n * (uint64_t) t / (uint64_t) nt;
    piece[t].last = n * (uint64_t) (t + 1) / (uint64_t) nt;
  }
  for (t = 1; t < nt; t++)
  {
    if (pthread_create(tid + t, NULL, work, piece + t) != 0)
    {
      break;
    }
    started = t;
  }
  (void) work(piece);
  for (t = started + 1; t < nt; t++) /* the pieces no thread took */
  {
    (void) work(piece + t);
  }
  for (t = 1; t <= started; t++)
  {
    (void) pthread_join(tid[t], NULL);
  }
  *npieces = nt;
}

/* ---- the two substrings of a record --------------------------------------- */

typedef struct
{
  int kind, palindromic;
  uint64_t n1;
  const uint8_t *text, *querysymbols;
  uint64_t numofqueries;
  const uint64_t *querystart, *querylength;
} Texts;

/* 0 and the view, the pair and the offset of v's first symbol in the query
   symbols (or the text), or -2 */
static int pairof(const Texts *x, const vsa_match *m, vsa_al_view *w,
                  vsa_al_pair *p, uint64_t *vfirst)
{
  uint64_t seqlength2 = 0;

  memset(p, 0, sizeof *p);
  if (!vsa_al_isself(x->kind))
  {
    if (m->queryseq >= x->numofqueries)
    {
      return -2;
    }
    seqlength2 = x->querylength[m->queryseq];
  }
  if (vsa_al_viewof(x->kind, m, seqlength2, w) != 0 ||
      !vsa_al_fits(w, m->dbstart, x->n1,
                   vsa_al_isself(x->kind) ? x->n1 : seqlength2))
  {
    return -2;
  }
  p->u = x->text + m->dbstart;
  p->ulen = w->length1;
  p->vlen = w->length2;
  if (vsa_al_isself(x->kind))
  {
    *vfirst = w->start2;
    p->v = x->text + w->start2;
    p->onearray = 1;
    p->pu = m->dbstart;
    p->pv = w->start2;
  } else
  {
    *vfirst = x->querystart[m->queryseq] +
              vsa_al_vfirst(w, seqlength2, x->palindromic);
    p->v = x->querysymbols + *vfirst;
    p->vrev = x->palindromic;
  }
  return 0;
}

/* what both entries refuse of a layout */
static int checklayout(const char *who, const vsa_sinkparams *layout,
                       const uint8_t *text, const uint8_t *querysymbols,
                       int palindromic, Texts *x)
{
  if (layout->selfpalindromic)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: lists of vmatch -p IDX "
                    "(selfpalindromic) are not covered", who);
  }
  if (!vsa_al_covered(layout->kind))
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: a layout of kind %d (X-drop "
                    "extended seeds, a six-frame translated batch) is not "
                    "covered", who, layout->kind);
  }
  if (layout->totallength == 0 || text == NULL ||
      (vsa_al_isself(layout->kind)
           ? palindromic != 0
           : (querysymbols == NULL ||
              (layout->numofqueries > 0 &&
               (layout->querystart == NULL || layout->querylength == NULL)))) ||
      (palindromic && layout->numofchars != 4))
  {
    return vsa_fail(-2, "%s: a query layout with the symbols of its batch "
                    "(palindromic: over 4 characters) or a self layout, not "
                    "palindromic", who);
  }
  x->kind = layout->kind;
  x->palindromic = palindromic != 0;
  x->n1 = layout->totallength;
  x->text = text;
  x->querysymbols = querysymbols;
  x->numofqueries = layout->numofqueries;
  x->querystart = layout->querystart;
  x->querylength = layout->querylength;
  return 0;
}

/* ---- the scripts ---------------------------------------------------------- */

typedef struct
{
  uint16_t *p;
  uint64_t len, cap;
} Words;

static int wordsroom(Words *w, uint64_t more)
{
  if (w->len + more > w->cap)
  {
    const uint64_t cap = 2 * w->cap + more + 1024;
    uint16_t *q = (uint16_t *) realloc(w->p, cap * sizeof *q);
    if (q == NULL)
    {
      return -1;
    }
    w->p = q;
    w->cap = cap;
  }
  return 0;
}

typedef struct
{
  int64_t *rows;  /* two fronts of 2 d + 3 rows: a minus infinity either side */
  uint8_t *dirs;  /* (d + 1) (2 d + 1) directions */
  uint64_t dist;  /* what they have room for */
} Fronts;

static int frontsroom(Fronts *f, uint64_t d)
{
  if (f->rows == NULL || d > f->dist)
  {
    free(f->rows);
    free(f->dirs);
    f->rows = (int64_t *) malloc(2 * (2 * d + 3) * sizeof *f->rows);
    f->dirs = (uint8_t *) malloc((d + 1) * (2 * d + 1));
    f->dist = d;
    if (f->rows == NULL || f->dirs == NULL)
    {
      return -1;
    }
  }
  return 0;
}

/* greedyedistalign with maxdist = d and backtracefront: the words of the
   script at out (room for vsa_al_maxwords) -> their number, -1 if the edit
   distance is above d */
static int64_t edistscript(const vsa_al_pair *p, uint64_t d, Fronts *f,
                           uint16_t *out)
{
  const int64_t D = (int64_t) d, width = 2 * D + 3;
  const int64_t enddiag = (int64_t) p->vlen - (int64_t) p->ulen;
  int64_t *prev = f->rows + 1 + D, *cur = f->rows + width + 1 + D, *swap;
  int64_t g, k, real = -1, i, j, dg, n = 0;

  for (k = -D - 1; k <= D + 1; k++)
  {
    prev[k] = cur[k] = VSA_ER_NEG;
  }
  prev[0] = vsa_al_slide(p, 0, 0);
  if (p->ulen == p->vlen && vsa_al_ends(prev[0], p->ulen))
  {
    real = 0;
  }
  for (g = 1; real < 0 && g <= D; g++)
  {
    for (k = -g; k <= g; k++)
    {
      int64_t t;
      f->dirs[g * (2 * D + 1) + k + D] =
          (uint8_t) vsa_al_direction(prev[k], prev[k - 1], prev[k + 1], &t);
      cur[k] = vsa_al_entry(p, t, k);
    }
    swap = prev;
    prev = cur;
    cur = swap;
    for (k = -D - 1; k <= D + 1; k++)
    {
      cur[k] = VSA_ER_NEG;
    }
    if (vsa_al_ends(prev[enddiag], p->ulen))
    {
      real = g;
    }
  }
  if (real < 0)
  {
    return -1;
  }
  dg = enddiag;
  i = (int64_t) p->ulen - 1;
  j = (int64_t) p->vlen - 1;
  for (g = real; g > 0; g--)
  {
    const int64_t run = vsa_al_slideback(p, i, j);
    i -= run;
    j -= run;
    if (run > 0)
    {
      n += (int64_t) vsa_al_identical(out + n, (uint64_t) run);
    }
    out[n++] = vsa_al_step(f->dirs[g * (2 * D + 1) + dg + D], &i, &j, &dg);
  }
  if (i >= 0)
  {
    n += (int64_t) vsa_al_identical(out + n, (uint64_t) i + 1);
  }
  return n;
}

typedef struct
{
  Texts x;
  const vsa_match *matches;
  uint64_t *counts; /* counts[i]: the words of record i */
} ScriptJob;

#define RC_DISTANCE (-20) /* the edit distance is above the stored one */

static void *scriptpiece(void *arg)
{
  Piece *pc = (Piece *) arg;
  const ScriptJob *job = (const ScriptJob *) pc->job;
  Words w = {NULL, 0, 0};
  Fronts f = {NULL, NULL, 0};
  uint64_t i;

  for (i = pc->first; i < pc->last && pc->rc == 0; i++)
  {
    vsa_al_view v;
    vsa_al_pair p;
    uint64_t vfirst, ad, n;

    pc->record = i;
    if (pairof(&job->x, job->matches + i, &v, &p, &vfirst) != 0)
    {
      pc->rc = -2;
      break;
    }
    ad = (uint64_t) (v.distance < 0 ? -v.distance : v.distance);
    if (v.distance > 0)
    {
      int64_t got;
      if (wordsroom(&w, vsa_al_maxwords(ad, p.ulen, p.vlen)) != 0 ||
          frontsroom(&f, ad) != 0)
      {
        pc->rc = -101;
        break;
      }
      got = edistscript(&p, ad, &f, w.p + w.len);
      if (got < 0)
      {
        pc->rc = RC_DISTANCE;
        break;
      }
      n = (uint64_t) got;
    } else
    {
      n = v.distance == 0 ? vsa_al_identical(NULL, p.ulen)
                          : vsa_al_hamming(&p, NULL);
      if (wordsroom(&w, n) != 0)
      {
        pc->rc = -101;
        break;
      }
      if (v.distance == 0)
      {
        (void) vsa_al_identical(w.p + w.len, p.ulen);
      } else
      {
        (void) vsa_al_hamming(&p, w.p + w.len);
      }
    }
    job->counts[i] = n;
    w.len += n;
  }
  free(f.rows);
  free(f.dirs);
  pc->out = w.p;
  pc->outlen = w.len;
  return NULL;
}

int vsa_align_host(const vsa_sinkparams *layout, const uint8_t *text,
                   const uint8_t *querysymbols, const vsa_match *matches,
                   uint64_t n, int palindromic, int threads,
                   uint64_t *offsets, uint16_t *eops, uint64_t capacity)
{
  static const char who[] = "vsa_align_host";
  Piece piece[MAXTHREADS];
  ScriptJob job;
  uint64_t i, total = 0;
  int t, np = 0, rc;

  if (layout == NULL || offsets == NULL || (eops == NULL && capacity > 0) ||
      (matches == NULL && n > 0))
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  offsets[0] = 0;
  if ((rc = checklayout(who, layout, text, querysymbols, palindromic,
                        &job.x)) != 0)
  {
    return rc;
  }
  if (n == 0)
  {
    return 0;
  }
  job.matches = matches;
  job.counts = offsets + 1;
  runpieces(scriptpiece, &job, n, threads, 256, piece, &np);
  for (t = 0; t < np && rc == 0; t++)
  {
    if (piece[t].rc == -101)
    {
      rc = vsa_fail(-101, "out of memory");
    } else if (piece[t].rc == RC_DISTANCE)
    {
      rc = vsa_fail(-2, "%s: the edit distance of record %lu is above the "
                    "distance it carries", who,
                    (unsigned long) piece[t].record);
    } else if (piece[t].rc != 0)
    {
      rc = vsa_list_misfit(who, piece[t].record);
    }
  }
  if (rc == 0)
  {
    for (i = 0; i < n; i++)
    {
      const uint64_t c = offsets[i + 1];
      offsets[i + 1] = total + c;
      total += c;
    }
    if (total > capacity)
    {
      rc = vsa_fail(-3, "%s: %lu words do not fit a buffer of %lu", who,
                    (unsigned long) total, (unsigned long) capacity);
    }
  }
  for (t = 0; t < np; t++)
  {
    if (rc == 0 && piece[t].outlen > 0)
    {
      memcpy(eops + offsets[piece[t].first], piece[t].out,
             piece[t].outlen * sizeof *eops);
    }
    free(piece[t].out);
  }
  return rc;
}

/* ---- the text ------------------------------------------------------------- */

typedef struct
{
  char *p;
  uint64_t len, cap;
} Text;

static char *textroom(Text *t, uint64_t more)
{
  if (t->len + more > t->cap)
  {
    const uint64_t cap = 2 * t->cap + more + 4096;
    char *q = (char *) realloc(t->p, cap);
    if (q == NULL)
    {
      return NULL;
    }
    t->p = q;
    t->cap = cap;
  }
  return t->p + t->len;
}

/* makereversecomplementorig, kurtz-basic/readmulti.c:55-79 */
static uint8_t complementorig(uint8_t c)
{
  switch (c)
  {
    case 'A': return 'T';
    case 'a': return 't';
    case 'C': return 'G';
    case 'c': return 'g';
    case 'G': return 'C';
    case 'g': return 'c';
    case 'T': return 'A';
    case 't': return 'a';
    default: return c;
  }
}

/* CHECKORIGEQUAL, showalign.c:1691-1704 */
static int origequal(uint8_t a, uint8_t b)
{
  if (a == b)
  {
    return 1;
  }
  return islower(a) ? a == (uint8_t) tolower(b) : a == (uint8_t) toupper(b);
}

static char *putnumber(char *o, uint64_t v, int width)
{
  return o + sprintf(o, "%*lu", width, (unsigned long) v);
}

typedef struct
{
  uint8_t *p; /* four lines of `cap` columns: compare 1, 2, original 1, 2 */
  uint64_t cap;
} Lines;

typedef struct
{
  Texts x;
  const vsa_sink *sink;
  const vsa_match *matches;
  const uint64_t *offsets;
  const uint16_t *eops;
  const uint8_t *origtext, *queryorig;
  uint64_t linewidth;
} FormatJob;

#define RC_SCRIPT (-21) /* the script does not account for its substrings */

/* showalignment for record m with the script words[0 .. nwords) */
static int showone(const FormatJob *job, const vsa_match *m,
                   const uint16_t *words, uint64_t nwords, Lines *ln, Text *t)
{
  const uint64_t W = job->linewidth;
  vsa_al_view v;
  vsa_al_pair p;
  uint64_t vfirst, cols = 0, i = 0, j = 0, c, ins1 = 0, ins2 = 0, done = 0;
  uint64_t startfirst, startsecond;
  const uint8_t *uorig, *vorig;
  uint8_t *fc, *sc, *fo, *so;
  int64_t e;
  const int self = vsa_al_isself(job->x.kind);

  if (pairof(&job->x, m, &v, &p, &vfirst) != 0)
  {
    return -2;
  }
  /* the columns of the script, and whether it accounts for u and v */
  for (e = 0; e < (int64_t) nwords; e++)
  {
    const uint16_t w = words[e];
    const uint64_t run = (w & ~VSA_AL_MAXRUN) == 0 ? w : 1;
    if (w == 0)
    {
      return RC_SCRIPT;
    }
    cols += run;
    i += w == VSA_AL_INSERTION ? 0 : run;
    j += w == VSA_AL_DELETION ? 0 : run;
  }
  if (i != p.ulen || j != p.vlen)
  {
    return RC_SCRIPT;
  }
  if (cols > ln->cap)
  {
    free(ln->p);
    ln->cap = cols + 1024;
    ln->p = (uint8_t *) malloc(4 * ln->cap);
    if (ln->p == NULL)
    {
      ln->cap = 0;
      return -101;
    }
  }
  fc = ln->p;
  sc = fc + ln->cap;
  fo = sc + ln->cap;
  so = fo + ln->cap;
  uorig = job->origtext + m->dbstart;
  vorig = (self ? job->origtext : job->queryorig) + vfirst;
  /* fillthelines: the last word is the first operation */
  i = j = c = 0;
  for (e = (int64_t) nwords - 1; e >= 0; e--)
  {
    const uint16_t w = words[e];
    uint64_t run = (w & ~VSA_AL_MAXRUN) == 0 ? w : 1;
    for (; run > 0; run--, c++)
    {
      if (w == VSA_AL_INSERTION)
      {
        fc[c] = fo[c] = GAPSYMBOL;
      } else
      {
        fc[c] = p.u[i];
        fo[c] = uorig[i];
        i++;
      }
      if (w == VSA_AL_DELETION)
      {
        sc[c] = so[c] = GAPSYMBOL;
      } else
      {
        sc[c] = vsa_al_vsym(&p, (int64_t) j);
        so[c] = p.vrev ? complementorig(*(vorig - j)) : vorig[j];
        j++;
      }
    }
  }
  startfirst = vsa_sink_relpos_(job->sink, m->dbstart);
  startsecond = self ? vsa_sink_relpos_(job->sink, v.start2)
                : job->x.palindromic
                    ? job->x.querylength[m->queryseq] -
                          (v.start2 + v.length2)
                    : v.start2;
  /* formatalignment */
  for (;;)
  {
    const uint64_t len = cols - done < W ? cols - done : W;
    const int numwidth = (int) (NUMWIDTH + W - len);
    char *o = textroom(t, 3 * (W + 64));
    uint64_t x;
    int marked = 0;

    if (o == NULL)
    {
      return -101;
    }
    memcpy(o, "Sbjct: ", 7);
    o += 7;
    for (x = done; x < done + len; x++)
    {
      ins1 += fo[x] == GAPSYMBOL;
      *o++ = fo[x] == GAPSYMBOL ? '-' : (char) fo[x];
    }
    o = putnumber(o, done + startfirst + len - ins1, numwidth);
    *o++ = '\n';
    /* showeditopline: only where the block has a difference */
    for (x = done; x < done + len && !marked; x++)
    {
      marked = fc[x] != sc[x] || fc[x] == GAPSYMBOL ||
               fc[x] == VSA_WILDCARD || !origequal(fo[x], so[x]);
    }
    if (marked)
    {
      memcpy(o, "       ", 7);
      o += 7;
      for (x = done; x < done + len; x++)
      {
        *o++ = (fc[x] != sc[x] || fc[x] == GAPSYMBOL ||
                fc[x] == VSA_WILDCARD)
                   ? '!'
                   : origequal(fo[x], so[x]) ? ' ' : '=';
      }
      *o++ = '\n';
    }
    memcpy(o, self ? "Sbjct: " : "Query: ", 7);
    o += 7;
    for (x = done; x < done + len; x++)
    {
      ins2 += so[x] == GAPSYMBOL;
      *o++ = so[x] == GAPSYMBOL ? '-' : (char) so[x];
    }
    o = putnumber(o, done + startsecond + len - ins2, numwidth);
    *o++ = '\n';
    done += len;
    /* the blank line between two blocks; behind the last one that of
       formatalignment and the one vmatch ends a match with */
    *o++ = '\n';
    if (done >= cols)
    {
      *o++ = '\n';
    }
    t->len = (uint64_t) (o - t->p);
    if (done >= cols)
    {
      return 0;
    }
  }
}

static void *formatpiece(void *arg)
{
  Piece *pc = (Piece *) arg;
  const FormatJob *job = (const FormatJob *) pc->job;
  Text t = {NULL, 0, 0};
  Lines ln = {NULL, 0};
  void *cache = vsa_sink_cache_new_();
  uint64_t i;

  if (cache == NULL)
  {
    pc->rc = -101;
  }
  for (i = pc->first; i < pc->last && pc->rc == 0; i++)
  {
    char *o = textroom(&t, VSA_SINK_LINEMAX), *e;

    pc->record = i;
    if (o == NULL)
    {
      pc->rc = -101;
      break;
    }
    e = vsa_sink_line_(job->sink, cache, job->matches + i, o);
    if (e == NULL)
    {
      pc->rc = -2;
      break;
    }
    if (e == o) /* the sink drops the match: no alignment either */
    {
      continue;
    }
    t.len += (uint64_t) (e - o);
    if (job->offsets[i + 1] < job->offsets[i])
    {
      pc->rc = RC_SCRIPT;
      break;
    }
    pc->rc = showone(job, job->matches + i, job->eops + job->offsets[i],
                     job->offsets[i + 1] - job->offsets[i], &ln, &t);
  }
  vsa_sink_cache_free_(cache);
  free(ln.p);
  pc->out = t.p;
  pc->outlen = t.len;
  return NULL;
}

#define ROUNDRECORDS (1u << 16) /* records per round of the threads */

static int formatall(const char *who, vsa_sink *sink,
                     const vsa_match *matches, uint64_t n,
                     const uint64_t *offsets, const uint16_t *eops,
                     const uint8_t *text, const uint8_t *origtext,
                     const uint8_t *querysymbols, const uint8_t *queryorig,
                     uint32_t linewidth,
                     int (*emit)(void *, const char *, uint64_t), void *info)
{
  const vsa_sinkparams *layout;
  FormatJob job;
  uint64_t done;
  int rc;

  if (sink == NULL || (n > 0 && (matches == NULL || offsets == NULL)) ||
      origtext == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  layout = vsa_sink_params_(sink);
  if ((rc = checklayout(who, layout, text, querysymbols, layout->palindromic,
                        &job.x)) != 0)
  {
    return rc;
  }
  if (!vsa_al_isself(layout->kind) && queryorig == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (linewidth > 1023) /* MAXLINEWIDTH, Vmatch/outinfo.h:51 */
  {
    return vsa_fail(-2, "%s: a line width of up to 1023 columns", who);
  }
  if (vsa_sink_prepare_(sink, matches, n) != 0)
  {
    return -101;
  }
  job.sink = sink;
  job.offsets = offsets;
  job.eops = eops;
  job.origtext = origtext;
  job.queryorig = queryorig;
  job.linewidth = linewidth == 0 ? DEFAULTLINEWIDTH : linewidth;
  for (done = 0; done < n && rc == 0; done += ROUNDRECORDS)
  {
    const uint64_t round = n - done < ROUNDRECORDS ? n - done : ROUNDRECORDS;
    Piece piece[MAXTHREADS];
    int t, np = 0;

    job.matches = matches + done;
    job.offsets = offsets + done;
    runpieces(formatpiece, &job, round, layout->threads > 0 ? layout->threads
                                                            : 0,
              512, piece, &np);
    for (t = 0; t < np; t++)
    {
      if (rc == 0 && piece[t].rc == -101)
      {
        rc = vsa_fail(-101, "out of memory");
      } else if (rc == 0 && piece[t].rc == RC_SCRIPT)
      {
        rc = vsa_fail(-2, "%s: the script of record %lu does not account "
                      "for its two substrings", who,
                      (unsigned long) (done + piece[t].record));
      } else if (rc == 0 && piece[t].rc != 0)
      {
        rc = vsa_list_misfit(who, done + piece[t].record);
      }
      if (rc == 0)
      {
        rc = emit(info, (const char *) piece[t].out, piece[t].outlen);
      }
      free(piece[t].out);
    }
  }
  return rc;
}

typedef struct
{
  char *buffer;
  uint64_t used, capacity;
} Membuf;

static int emitmemory(void *info, const char *text, uint64_t len)
{
  Membuf *mb = (Membuf *) info;

  if (mb->used + len > mb->capacity)
  {
    return vsa_fail(-3, "vsa_align_format: buffer of %lu bytes is too small",
                    (unsigned long) mb->capacity);
  }
  if (len > 0)
  {
    memcpy(mb->buffer + mb->used, text, (size_t) len);
  }
  mb->used += len;
  return 0;
}

static int emitfile(void *info, const char *text, uint64_t len)
{
  if (len > 0 && fwrite(text, 1, (size_t) len, (FILE *) info) != (size_t) len)
  {
    return vsa_fail(-4, "vsa_align_write: write failed");
  }
  return 0;
}

int64_t vsa_align_format(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                         const uint64_t *offsets, const uint16_t *eops,
                         const uint8_t *text, const uint8_t *origtext,
                         const uint8_t *querysymbols,
                         const uint8_t *queryorig, uint32_t linewidth,
                         char *buffer, uint64_t capacity)
{
  Membuf mb;
  int rc;

  if (capacity > 0 && buffer == NULL)
  {
    return vsa_fail(-1, "vsa_align_format: NULL argument");
  }
  mb.buffer = buffer;
  mb.used = 0;
  mb.capacity = capacity;
  rc = formatall("vsa_align_format", sink, matches, n, offsets, eops, text,
                 origtext, querysymbols, queryorig, linewidth, emitmemory,
                 &mb);
  return rc != 0 ? (int64_t) rc : (int64_t) mb.used;
}

int vsa_align_write(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                    const uint64_t *offsets, const uint16_t *eops,
                    const uint8_t *text, const uint8_t *origtext,
                    const uint8_t *querysymbols, const uint8_t *queryorig,
                    uint32_t linewidth, void *file)
{
  if (file == NULL)
  {
    return vsa_fail(-1, "vsa_align_write: NULL argument");
  }
  return formatall("vsa_align_write", sink, matches, n, offsets, eops, text,
                   origtext, querysymbols, queryorig, linewidth, emitfile,
                   file);
}
