/*
  Match selection, host side (plain C): the description of a selection with
  the tables the kernels of select.hip read, the -sort tail on the at most N
  survivors, and vsa_select_host -- the same rules on a list in host memory,
  without a GPU.

  Restates
    matchokay            Vmatch/mokay.c:7-114            (select_rules.h)
    assignEvalue         Vmatch/procfinal.c:195-257      (select_rules.h)
    insertintobml        kurtz/bestmatch.c:33-189 with insertDictmaxsize,
                         kurtz-basic/dictmaxsize.c: the N best distinct
                         matches under cmpBestMatch -- a total order, so the
                         outcome does not depend on the order of insertion
    showbestmatchlist    Vmatch/procfinal.c:695-745
    removecontained      kurtz/smcontain.c:23-95
    sortallmatches       kurtz/matsort.c:28-180,249-263
  The reference sorts with glibc's qsort, a stable merge sort; msort() below
  merges the same way (the left run wins where the comparison says <= 0), so
  the comparison functions can stay the reference's, ties included.
*/
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "select_internal.h"
#include "host_common.h"

/* ---- the description of a selection ----------------------------------- */

static int isapprox(int kind)
{
  return kind == VSA_SINK_APPROX_EDIST || kind == VSA_SINK_APPROX_HAMMING;
}

static int settables(vsa_selctx *ctx, int64_t nlines)
{
  int64_t d;
  double *h;

  if (vsa_evalues_extend(&ctx->ev, nlines - 1) != 0 ||
      (h = (double *) realloc(ctx->hequot,
                              (size_t) nlines * sizeof(double))) == NULL)
  {
    return vsa_fail(-101, "out of memory");
  }
  for (d = 0; d < nlines; d++)
  {
    h[d] = d <= VSA_EVALUES_MAXEDIST ? vsa_evalues_hequot(d) : 0.0;
  }
  ctx->hequot = h;
  ctx->rules.hequot = h;
  ctx->rules.table = ctx->ev.table;
  ctx->rules.linestart = ctx->ev.linestart;
  ctx->rules.nlines = nlines;
  return 0;
}

int vsa_selctx_init(vsa_selctx *ctx, const vsa_sinkparams *layout,
                    const vsa_selectparams *params, uint64_t nq,
                    const uint64_t *qstart, const uint64_t *qlen,
                    uint32_t uniformlen, uint64_t seqoffset)
{
  static const char who[] = "vsa_select";
  vsa_selrules *r = &ctx->rules;
  const uint64_t dblen = layout->totallength - layout->totalquerylength - 1;
  int rc;

  memset(ctx, 0, sizeof *ctx);
  /* (the query arrays are the caller's: their refusal comes below) */
  if ((rc = vsa_layout_view(layout, who, VSA_NEEDS_CHARS, r)) != 0)
  {
    return rc;
  }
  if (params->sortmode < 0 || params->sortmode > VSA_SORT_NONE)
  {
    return vsa_fail(-2, "%s: illegal sort mode %d", who, params->sortmode);
  }
  if (params->sortmode != VSA_SORT_NONE && params->bestnumber == 0)
  {
    /* Vmatch/parsevm.c: -sort goes with -best */
    return vsa_fail(-2, "%s: a sort mode needs bestnumber > 0", who);
  }
  if (params->bestnumber > 0xFFFFFFF0ull)
  {
    return vsa_fail(-2, "%s: bestnumber %lu is beyond 2^32 - 16", who,
                    (unsigned long) params->bestnumber);
  }
  if (params->identity > 100 ||
      (params->hasleastscore && params->leastscore < 0))
  {
    return vsa_fail(-2, "%s: identity must be 0..100, leastscore >= 0", who);
  }
  if ((params->haslowergap || params->hasuppergap) &&
      layout->kind != VSA_SINK_SELF)
  {
    return vsa_fail(-2, "%s: gap bounds go with matches of the index against "
                    "itself (VSA_SINK_SELF)", who);
  }
  if (params->hasuppergap && !params->haslowergap)
  {
    return vsa_fail(-2, "%s: the upper gap bound needs the lower one", who);
  }
  if (layout->kind != VSA_SINK_SELF && nq > 0 && uniformlen == 0 &&
      (qstart == NULL || qlen == NULL))
  {
    return vsa_fail(-2, "%s: the layout has no query Multiseq", who);
  }
  /* what the view leaves to a selection: E-values, and the query Multiseq
     of the batch in copies of its own */
  ctx->params = *params;
  r->noevalue = (layout->showmode & VSA_SHOW_NOEVALUE) != 0;
  r->leastlength = layout->leastlength;
  if (layout->kind == VSA_SINK_SELF)
  {
    r->multiplier = r->hasindexedqueries
                        ? (double) dblen * (double) layout->totalquerylength
                        : 0.5 * (double) layout->totallength *
                              (double) layout->totallength;
  } else
  {
    r->multiplier = (double) layout->totallength;
    r->nq = nq;
    r->seqoffset = seqoffset;
    r->uniformlen = uniformlen;
    r->qstart = r->qlen = NULL;
    if (uniformlen == 0 && nq > 0)
    {
      ctx->qstart = (uint64_t *) malloc((size_t) nq * 8);
      ctx->qlen = (uint64_t *) malloc((size_t) nq * 8);
      if (ctx->qstart == NULL || ctx->qlen == NULL)
      {
        vsa_selctx_free(ctx);
        return vsa_fail(-101, "out of memory");
      }
      memcpy(ctx->qstart, qstart, (size_t) nq * 8);
      memcpy(ctx->qlen, qlen, (size_t) nq * 8);
      r->qstart = ctx->qstart;
      r->qlen = ctx->qlen;
    }
  }
  r->hasmaxevalue = params->hasmaxevalue;
  r->maximumevalue = params->maximumevalue;
  r->identity = params->identity;
  r->hasleastscore = params->hasleastscore;
  r->leastscore = params->leastscore;
  r->haslowergap = params->haslowergap;
  r->hasuppergap = params->hasuppergap;
  r->lowergap = params->lowergap;
  r->uppergap = params->uppergap;
  vsa_evalues_init(&ctx->ev, layout->numofchars);
  if (settables(ctx, isapprox(layout->kind) ? 21 : 1) != 0)
  {
    vsa_selctx_free(ctx);
    return -101;
  }
  return 0;
}

void vsa_selctx_free(vsa_selctx *ctx)
{
  vsa_evalues_free(&ctx->ev);
  free(ctx->hequot);
  free(ctx->qstart);
  free(ctx->qlen);
  memset(ctx, 0, sizeof *ctx);
}

int vsa_selctx_ensure(vsa_selctx *ctx, uint64_t maxdistance)
{
  /* an edit distance beyond the limit has the E-value 0.0 without a look at
     the table (kurtz/evalues.c:402-407); a Hamming distance reads its line */
  if (ctx->rules.kind == VSA_SINK_APPROX_EDIST &&
      maxdistance > VSA_EVALUES_MAXEDIST)
  {
    maxdistance = VSA_EVALUES_MAXEDIST;
  }
  if (!isapprox(ctx->rules.kind) || ctx->rules.noevalue ||
      (int64_t) maxdistance < ctx->rules.nlines)
  {
    return 0;
  }
  if (maxdistance > 1u << 20)
  {
    return vsa_fail(-2, "vsa_select: a distance of %lu",
                    (unsigned long) maxdistance);
  }
  return settables(ctx, (int64_t) maxdistance + 1) != 0 ? -101 : 1;
}

/* ---- glibc's qsort: a merge sort that takes the left run on <= 0 ------- */

typedef int (*Cmp)(const void *, const void *, const void *);

static void msort(char *b, size_t n, size_t size, Cmp cmp, const void *info,
                  char *tmp)
{
  size_t n1, n2;
  char *b1, *b2, *t = tmp;

  if (n <= 1)
  {
    return;
  }
  n1 = n / 2;
  n2 = n - n1;
  b1 = b;
  b2 = b + n1 * size;
  msort(b1, n1, size, cmp, info, tmp);
  msort(b2, n2, size, cmp, info, tmp);
  while (n1 > 0 && n2 > 0)
  {
    if (cmp(b1, b2, info) <= 0)
    {
      memcpy(t, b1, size);
      b1 += size;
      n1--;
    } else
    {
      memcpy(t, b2, size);
      b2 += size;
      n2--;
    }
    t += size;
  }
  if (n1 > 0)
  {
    memcpy(t, b1, n1 * size);
  }
  memcpy(b, tmp, (n - n2) * size);
}

static int stablesort(void *base, size_t n, size_t size, Cmp cmp,
                      const void *info)
{
  char *tmp;

  if (n <= 1)
  {
    return 0;
  }
  tmp = (char *) malloc(n * size);
  if (tmp == NULL)
  {
    return vsa_fail(-101, "out of memory");
  }
  msort((char *) base, n, size, cmp, info, tmp);
  free(tmp);
  return 0;
}

/* ---- the -sort tail ---------------------------------------------------- */

typedef struct
{
  vsa_match rec;
  vsa_selvalues v;
  uint8_t flag;
} Stored;

/* ordermatchp1l1, kurtz/smcontain.c:23-34 */
static int ordermatchp1l1(const void *a, const void *b, const void *info)
{
  const Stored *p = (const Stored *) a, *q = (const Stored *) b;

  (void) info;
  if (p->v.position1 == q->v.position1)
  {
    if (p->v.length1 == q->v.length1)
    {
      return (p->v.position2 > q->v.position2) ? 1 : -1;
    }
    return (p->v.length1 > q->v.length1) ? 1 : -1;
  }
  return (p->v.position1 > q->v.position1) ? 1 : -1;
}

/* CONTAINSSTOREMATCH, include/match.h:156-162 */
static int contains(const Stored *m1, const Stored *m2)
{
  return m1->v.position1 <= m2->v.position1 &&
         m2->v.position1 + m2->v.length1 <= m1->v.position1 + m1->v.length1 &&
         m1->v.position2 <= m2->v.position2 &&
         m2->v.position2 + m2->v.length2 <= m1->v.position2 + m1->v.length2;
}

/* removecontained, kurtz/smcontain.c:41-95 */
static int64_t removecontained(Stored *tab, uint64_t n, uint64_t *removed)
{
  uint8_t *reject;
  uint64_t i, kept = 0;
  Stored *mptr1, *mptr2;

  *removed = 0;
  if (n == 0)
  {
    return 0;
  }
  if (stablesort(tab, (size_t) n, sizeof(Stored), ordermatchp1l1, NULL) != 0)
  {
    return -101;
  }
  reject = (uint8_t *) calloc((size_t) n, 1);
  if (reject == NULL)
  {
    return vsa_fail(-101, "out of memory");
  }
  for (mptr1 = tab; mptr1 < tab + n; mptr1++)
  {
    const uint64_t idxaux = (uint64_t) (mptr1 - tab);
    for (mptr2 = mptr1 - 1;
         mptr2 >= tab && mptr2->v.position1 == mptr1->v.position1; mptr2--)
    {
      if (!reject[idxaux] && contains(mptr1, mptr2))
      {
        reject[mptr2 - tab] = 1;
      }
    }
    for (mptr2 = mptr1 + 1;
         mptr2 < tab + n &&
         mptr2->v.position1 <= mptr1->v.position1 + mptr1->v.length1;
         mptr2++)
    {
      if (!reject[idxaux] && contains(mptr1, mptr2))
      {
        reject[mptr2 - tab] = 1;
      }
    }
  }
  for (i = 0; i < n; i++)
  {
    if (!reject[i])
    {
      tab[kept++] = tab[i];
    }
  }
  free(reject);
  *removed = n - kept;
  return (int64_t) kept;
}

/* the comparison functions of kurtz/matsort.c:28-180 */
static int cmpu64(uint64_t p, uint64_t q, int ascend)
{
  if (p == q)
  {
    return 0;
  }
  return ((p > q) == (ascend != 0)) ? 1 : -1;
}

static int cmpdouble(double p, double q, int ascend)
{
  if (p == q)
  {
    return 0;
  }
  return ((p > q) == (ascend != 0)) ? 1 : -1;
}

static int cmpmode(const void *a, const void *b, const void *info)
{
  const Stored *p = (const Stored *) a, *q = (const Stored *) b;
  const int mode = *(const int *) info, ascend = (mode & 1) == 0;

  switch (mode >> 1)
  {
    case 0:
      return cmpu64(p->v.length1, q->v.length1, ascend);
    case 1:
      return cmpu64(p->v.position1, q->v.position1, ascend);
    case 2:
      return cmpu64(p->v.position2, q->v.position2, ascend);
    case 3:
      return cmpdouble(p->v.evalue, q->v.evalue, ascend);
    case 4:
    {
      /* cmpScoregeneric: equal scores are equal, otherwise the absolute
         values decide -- and equal absolute values of different sign order
         like "not greater" */
      int64_t sp = vsa_sel_score(&p->v), sq = vsa_sel_score(&q->v);
      if (sp == sq)
      {
        return 0;
      }
      sp = sp < 0 ? -sp : sp;
      sq = sq < 0 ? -sq : sq;
      return ascend ? ((sp > sq) ? 1 : -1) : ((sp > sq) ? -1 : 1);
    }
    default:
    {
      /* cmpIdentitygeneric */
      double ip = vsa_sel_identity(&p->v), iq = vsa_sel_identity(&q->v);
      if (ip == iq)
      {
        return 0;
      }
      ip = ip < 0.0 ? -ip : ip;
      iq = iq < 0.0 ? -iq : iq;
      return ascend ? ((ip > iq) ? 1 : -1) : ((ip > iq) ? -1 : 1);
    }
  }
}

int64_t vsa_select_sorttail(const vsa_selctx *ctx, vsa_match *matches,
                            uint8_t *flags, double *evalues, uint64_t n,
                            uint64_t *contained)
{
  Stored *tab;
  uint64_t i;
  int64_t kept;
  const int mode = ctx->params.sortmode;

  *contained = 0;
  if (n == 0 || mode == VSA_SORT_NONE)
  {
    return (int64_t) n;
  }
  tab = (Stored *) malloc((size_t) n * sizeof(Stored));
  if (tab == NULL)
  {
    return vsa_fail(-101, "out of memory");
  }
  for (i = 0; i < n; i++)
  {
    tab[i].rec = matches[i];
    tab[i].flag = flags[i];
    if (vsa_sel_values(&ctx->rules, matches + i, flags[i], &tab[i].v) != 0)
    {
      free(tab);
      return vsa_fail(-2, "vsa_select: a selected record does not fit the "
                      "layout");
    }
    tab[i].v.evalue = evalues[i];
  }
  kept = removecontained(tab, n, contained);
  /* mode 2, ia: the order removecontained left (procfinal.c:729) */
  if (kept > 0 && mode != 2 &&
      stablesort(tab, (size_t) kept, sizeof(Stored), cmpmode, &mode) != 0)
  {
    kept = -101;
  }
  for (i = 0; kept > 0 && i < (uint64_t) kept; i++)
  {
    matches[i] = tab[i].rec;
    flags[i] = tab[i].flag;
    evalues[i] = tab[i].v.evalue;
  }
  free(tab);
  return kept;
}

/* ---- the whole selection on the host ----------------------------------- */

typedef struct
{
  uint64_t key[VSA_SELECT_KEYWORDS];
  uint64_t idx;
} Keyed;

static int cmpkeyed(const void *a, const void *b, const void *info)
{
  (void) info;
  return vsa_sel_keycmp(((const Keyed *) a)->key, ((const Keyed *) b)->key);
}

int vsa_select_host(const vsa_sinkparams *layout,
                    const vsa_selectparams *params, const vsa_match *matches,
                    const uint8_t *palindromic, uint64_t n,
                    vsa_match *selected, uint8_t *selectedflags,
                    double *evalues, uint64_t capacity, uint64_t *nselected,
                    vsa_selectstats *stats)
{
  static const char who[] = "vsa_select";
  vsa_selctx ctx;
  vsa_selectstats st;
  Keyed *tab = NULL;
  uint8_t *oflags = NULL;
  double *oev = NULL;
  uint64_t i, m = 0, nout = 0, maxd = 0;
  int rc;

  if (layout == NULL || params == NULL || nselected == NULL ||
      (n > 0 && matches == NULL) || (capacity > 0 && selected == NULL))
  {
    return vsa_fail(-1, "vsa_select_host: NULL argument");
  }
  *nselected = 0;
  memset(&st, 0, sizeof st);
  /* (the handle takes such lists: the refusal is not vsa_selctx_init's) */
  if (vsa_layout_selfpalindromic(layout, who) != 0)
  {
    return VSA_NOT_COVERED;
  }
  rc = vsa_selctx_init(&ctx, layout, params, layout->numofqueries,
                       layout->querystart, layout->querylength, 0, 0);
  if (rc != 0)
  {
    return rc;
  }
  for (i = 0; i < n; i++)
  {
    int pal;
    if ((rc = vsa_list_flag(who, layout->kind, palindromic, i, &pal)) != 0)
    {
      vsa_selctx_free(&ctx);
      return rc;
    }
    if (isapprox(layout->kind) && matches[i].querystart > maxd)
    {
      maxd = matches[i].querystart;
    }
  }
  rc = vsa_selctx_ensure(&ctx, maxd);
  tab = (Keyed *) malloc((size_t) (n + 1) * sizeof(Keyed));
  oflags = (uint8_t *) malloc((size_t) n + 1);
  oev = (double *) malloc((size_t) (n + 1) * sizeof(double));
  if (rc >= 0 && (tab == NULL || oflags == NULL || oev == NULL))
  {
    rc = vsa_fail(-101, "out of memory");
  }
  for (i = 0; rc >= 0 && i < n; i++)
  {
    vsa_selvalues v;
    const int pal = palindromic != NULL && palindromic[i];
    if (vsa_sel_values(&ctx.rules, matches + i, pal, &v) != 0)
    {
      rc = vsa_list_misfit(who, i);
      break;
    }
    st.seen++;
    if (!vsa_sel_okay(&ctx.rules, &v))
    {
      st.rejected++;
      continue;
    }
    vsa_sel_key(&v, pal, tab[m].key);
    tab[m++].idx = i;
  }
  if (rc >= 0)
  {
    rc = 0;
  }
  if (rc == 0 && params->bestnumber > 0)
  {
    /* the N best distinct keys; of equal ones the first seen stays */
    rc = stablesort(tab, (size_t) m, sizeof(Keyed), cmpkeyed, NULL);
    if (rc == 0)
    {
      uint64_t k = 0;
      for (i = 0; i < m; i++)
      {
        if (k > 0 && vsa_sel_keycmp(tab[k - 1].key, tab[i].key) == 0)
        {
          st.duplicates++;
        } else if (k == params->bestnumber)
        {
          break;
        } else
        {
          tab[k++] = tab[i];
        }
      }
      m = k;
    }
  }
  if (rc == 0 && m > capacity)
  {
    rc = vsa_fail(-3, "vsa_select_host: %lu records for a capacity of %lu",
                  (unsigned long) m, (unsigned long) capacity);
  }
  if (rc == 0)
  {
    int64_t kept;
    for (i = 0; i < m; i++)
    {
      double e;
      selected[i] = matches[tab[i].idx];
      oflags[i] = (uint8_t) (tab[i].key[4] & 1u);
      memcpy(&e, &tab[i].key[0], 8);
      oev[i] = e;
    }
    kept = vsa_select_sorttail(&ctx, selected, oflags, oev, m,
                               &st.containedremoved);
    if (kept < 0)
    {
      rc = (int) kept;
    } else
    {
      nout = (uint64_t) kept;
    }
  }
  if (rc == 0)
  {
    if (selectedflags != NULL)
    {
      memcpy(selectedflags, oflags, (size_t) nout);
    }
    if (evalues != NULL)
    {
      memcpy(evalues, oev, (size_t) nout * sizeof(double));
    }
    st.selected = nout;
    *nselected = nout;
    if (stats != NULL)
    {
      *stats = st;
    }
  }
  free(tab);
  free(oflags);
  free(oev);
  vsa_selctx_free(&ctx);
  return rc;
}
