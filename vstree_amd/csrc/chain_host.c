/*
  Chaining, host side: a fresh restatement of vmatchchaining with its grouping
  (Vmatch/chainvm.c:180-500, groupmatchesbyseqnum of kurtz/matsort.c:316-367
  with the quicksort of include/qsort.gen), of the sweep of fastchaining
  (kurtz-basic/chain2dim.c:1436-1543,1659-1778) with a sorted array in the
  place of the red-black tree, of the brute-force scores of global ov
  (:776-888), of the retrieval (:1150-1360,1545-1657) and of the text
  (chainvm.c:106-161).  What a fragment is and how one is scored from its
  predecessor is chain_rules.h, the same text the kernels compile; here the
  predecessor comes out of the literal sweep, there out of the rule without
  an order of events.  No GPU involved.
*/
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "chain_rules.h"
#include "host_common.h"

int vsa_ch_checklayout(const vsa_sinkparams *layout,
                       const vsa_chainparams *params, const char *who,
                       vsa_selrules *rules, vsa_clrules *seqs)
{
  int rc;

  if (layout == NULL || params == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (params->thread)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: chain thread (closing the gaps of "
                    "a chain) is not covered", who);
  }
  if (params->kind < VSA_CHAIN_GLOBAL || params->kind > VSA_CHAIN_LOCAL_PERCENT)
  {
    return vsa_fail(-2, "%s: illegal kind %d", who, params->kind);
  }
  if (!(params->weightfactor > 0.0))
  {
    return vsa_fail(-2, "%s: the weight factor must be positive", who);
  }
  if (params->kind == VSA_CHAIN_LOCAL_BEST && params->value < 1)
  {
    return vsa_fail(-2, "%s: local Kb needs K >= 1", who);
  }
  if ((rc = vsa_layout_view(layout, who, VSA_NEEDS_NOSELFPAL |
                            VSA_NEEDS_SEQUENCES | VSA_NEEDS_QUERIES,
                            rules)) != 0)
  {
    return rc;
  }
  memset(seqs, 0, sizeof *seqs);
  seqs->totallength = layout->totallength;
  seqs->numofsequences = layout->numofsequences;
  seqs->markpos = layout->markpos;
  return 0;
}

/* outvmatchchain, chainvm.c:137-151 */
int64_t vsa_chain_format_host(vsa_sink *sink, int flags, uint64_t nchains,
                              const uint64_t *number, const int64_t *score,
                              const uint64_t *start, const vsa_match *records,
                              char *buffer, uint64_t capacity)
{
  vsa_textbuf t = {buffer, capacity, 0};
  char line[512];
  uint64_t c, k;

  if (sink == NULL || buffer == NULL ||
      (nchains > 0 && (number == NULL || score == NULL || start == NULL ||
                       records == NULL)))
  {
    return vsa_fail(-1, "vsa_chain_format_host: NULL argument");
  }
  for (c = 0; c < nchains; c++)
  {
    vsa_putf(&t, "# chain %lu: length %lu score %ld\n",
             (unsigned long) number[c],
             (unsigned long) (start[c + 1] - start[c]), (long) score[c]);
    if (flags & VSA_CHAIN_SILENT)
    {
      continue;
    }
    for (k = start[c]; k < start[c + 1]; k++)
    {
      const int64_t w = vsa_sink_format(sink, records + k, 1, line,
                                        sizeof line);
      if (w < 0)
      {
        return w;
      }
      vsa_put(&t, line, (size_t) w);
    }
  }
  return vsa_endtext(&t, "vsa_chain_format");
}

/* ---- sorting --------------------------------------------------------------- */

/* a merge sort of the indices a[0 .. n) by key[a[.]] that takes the left run
   on ties: stable, like the reference's counting sort and glibc's qsort */
static void sortidx(uint32_t *a, uint32_t *tmp, uint64_t n,
                    const uint64_t *key)
{
  uint64_t width, lo;

  for (width = 1; width < n; width *= 2)
  {
    for (lo = 0; lo < n; lo += 2 * width)
    {
      const uint64_t mid = lo + width < n ? lo + width : n,
                     hi = lo + 2 * width < n ? lo + 2 * width : n;
      uint64_t i = lo, j = mid, k = lo;
      while (i < mid && j < hi)
      {
        tmp[k++] = key[a[j]] < key[a[i]] ? a[j++] : a[i++];
      }
      while (i < mid)
      {
        tmp[k++] = a[i++];
      }
      while (j < hi)
      {
        tmp[k++] = a[j++];
      }
    }
    memcpy(a, tmp, (size_t) n * sizeof *a);
  }
}

#define SWAP(X, Y)                                                             \
  do                                                                           \
  {                                                                            \
    const uint32_t swaptmp = perm[X];                                          \
    perm[X] = perm[Y];                                                         \
    perm[Y] = swaptmp;                                                         \
  } while (0)

/* the quicksort of include/qsort.gen on perm[left .. right] by
   key[perm[.]]: median of three, the pivot parked at right - 1, runs of at
   most VSA_CH_STABLEWIDTH entries by an insertion sort that keeps the order
   of equal keys.  Wider runs get their equal keys shuffled, always in the
   same way.  0, or -1 without memory for the stack. */
static int groupquicksort(uint32_t *perm, int64_t left, int64_t right,
                          const uint64_t *key)
{
  int64_t *stack = NULL, i, j, k, mid;
  size_t top = 0, size = 0;

  for (;;)
  {
    const int64_t width = right - left + 1;
    if (width > (int64_t) VSA_CH_STABLEWIDTH)
    {
      uint64_t pivot;
      mid = left + ((right - left) >> 1);
      if (key[perm[left]] > key[perm[mid]])
      {
        SWAP(left, mid);
      }
      if (key[perm[mid]] > key[perm[right]])
      {
        SWAP(mid, right);
      }
      if (key[perm[left]] > key[perm[mid]])
      {
        SWAP(left, mid);
      }
      SWAP(mid, right - 1);
      pivot = key[perm[right - 1]];
      i = left;
      j = right - 1;
      for (;;)
      {
        do
        {
          i++;
        } while (key[perm[i]] < pivot);
        do
        {
          j--;
        } while (pivot < key[perm[j]]);
        if (i >= j)
        {
          break;
        }
        SWAP(i, j);
      }
      SWAP(i, right - 1);
      if (top + 2 > size)
      {
        int64_t *s = realloc(stack, (size + 128) * sizeof *s);
        if (s == NULL)
        {
          free(stack);
          return -1;
        }
        stack = s;
        size += 128;
      }
      if (i - left > right - i)
      {
        stack[top++] = left;
        stack[top++] = i - 1;
        left = i + 1;
      } else
      {
        stack[top++] = i + 1;
        stack[top++] = right;
        right = i - 1;
      }
      continue;
    }
    if (width == 2)
    {
      if (key[perm[left]] > key[perm[right]])
      {
        SWAP(left, right);
      }
    } else if (width > 2)
    {
      for (i = left + 1; i <= right; i++)
      {
        const uint32_t item = perm[i];
        k = i;
        for (;;)
        {
          if (key[item] >= key[perm[k - 1]])
          {
            break;
          }
          perm[k] = perm[k - 1];
          if (--k == left)
          {
            break;
          }
        }
        perm[k] = item;
      }
    }
    if (top == 0)
    {
      free(stack);
      return 0;
    }
    right = stack[--top];
    left = stack[--top];
  }
}

int vsa_ch_grouprank(const uint64_t *seq1, const uint64_t *seq2,
                     const uint32_t *recnum, uint64_t n, uint32_t *rank)
{
  uint32_t *perm = malloc((size_t) (n + 1) * sizeof *perm),
           *tmp = malloc((size_t) (n + 1) * sizeof *tmp);
  uint64_t *num = calloc((size_t) n + 1, sizeof *num);
  uint64_t i, first = 0;
  int rc = 0;

  if (perm == NULL || tmp == NULL || num == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  for (i = 0; i < n; i++)
  {
    perm[i] = (uint32_t) i;
    num[i] = recnum[i];
  }
  /* the counting sort leaves every run in the order of the record numbers */
  sortidx(perm, tmp, n, num);
  sortidx(perm, tmp, n, seq1);
  for (i = 1; i <= n; i++)
  {
    if (i == n || seq1[perm[i - 1]] != seq1[perm[i]])
    {
      if (first + 1 < i &&
          groupquicksort(perm, (int64_t) first, (int64_t) i - 1, seq2) != 0)
      {
        rc = vsa_fail(-1, "out of memory");
        goto done;
      }
      first = i;
    }
  }
  for (i = 0; i < n; i++)
  {
    rank[perm[i]] = (uint32_t) i;
  }
done:
  free(perm);
  free(tmp);
  free(num);
  return rc;
}

/* ---- one problem ------------------------------------------------------------ */

typedef struct
{
  const vsa_chainparams *r;
  uint64_t n;
  const vsa_chfrag *f; /* in the order of the fragments                     */
  int64_t *tg, *score, *cbest;
  uint32_t *prev, *first, *perm, *tmp, *tree;
  uint64_t *key; /* scratch: n words                                        */
  uint8_t *avail;
  uint64_t ntree;
} Problem;

/* the last place of the tree with a key not above (e0, num), or -1 */
static int64_t treefloor(const Problem *p, uint64_t e0, uint32_t num)
{
  int64_t lo = 0, hi = (int64_t) p->ntree;
  while (lo < hi)
  {
    const int64_t mid = lo + (hi - lo) / 2;
    const uint32_t j = p->tree[mid];
    if (p->f[j].e0 < e0 || (p->f[j].e0 == e0 && j <= num))
    {
      lo = mid + 1;
    } else
    {
      hi = mid;
    }
  }
  return lo - 1;
}

static void candidate(const Problem *p, uint32_t j, vsa_chcand *c)
{
  c->s0 = p->f[j].s0;
  c->e0 = p->f[j].e0;
  c->s1 = p->f[j].s1;
  c->e1 = p->f[j].e1;
  c->score = p->score[j];
  c->tg = p->tg[j];
  c->first = p->first[j];
}

/* evalfragmentscore: the predecessor is the tree's entry below the start */
static void evaluate(Problem *p, uint32_t i)
{
  vsa_chbest b;
  memset(&b, 0, sizeof b);
  if (p->f[i].s0 != 0)
  {
    const int64_t at = treefloor(p, p->f[i].s0 - 1, i);
    if (at >= 0)
    {
      const uint32_t j = p->tree[at];
      b.has = b.link = 1;
      b.key = vsa_ch_priority(p->score[j], p->tg[j]);
      b.score = p->score[j];
      b.e0 = p->f[j].e0;
      b.e1 = p->f[j].e1;
      b.j = j;
      b.first = p->first[j];
    }
  }
  vsa_ch_settle(p->r, &b, p->f + i, i, p->score + i, p->prev + i,
                p->first + i);
}

/* activatefragpoint, chain2dim.c:990-1049 */
static void activate(Problem *p, uint32_t j)
{
  const int64_t q = vsa_ch_priority(p->score[j], p->tg[j]);
  const int64_t at = treefloor(p, p->f[j].e0, j);
  uint64_t from, to;

  if (at >= 0 &&
      !(q > vsa_ch_priority(p->score[p->tree[at]], p->tg[p->tree[at]])))
  {
    return;
  }
  /* the successors of smaller priority go */
  from = to = (uint64_t) (at + 1);
  while (to < p->ntree &&
         vsa_ch_priority(p->score[p->tree[to]], p->tg[p->tree[to]]) < q)
  {
    to++;
  }
  if (to != from + 1)
  {
    memmove(p->tree + from + 1, p->tree + to,
            (size_t) (p->ntree - to) * sizeof *p->tree);
  }
  p->tree[from] = j;
  p->ntree = p->ntree - (to - from) + 1;
}

/* mergestartandendpoints -> the score of the entry with the greatest key */
static int64_t sweep(Problem *p)
{
  uint64_t s = 0, e = 0, i;

  for (i = 0; i < p->n; i++)
  {
    p->perm[i] = (uint32_t) i;
    p->key[i] = p->f[i].e1;
  }
  sortidx(p->perm, p->tmp, p->n, p->key);
  p->ntree = 0;
  while (s < p->n && e < p->n)
  {
    if (!vsa_ch_active(p->f[p->perm[e]].e1, p->f[s].s1))
    {
      evaluate(p, (uint32_t) s++);
    } else
    {
      activate(p, p->perm[e++]);
    }
  }
  while (s < p->n)
  {
    evaluate(p, (uint32_t) s++);
  }
  while (e < p->n)
  {
    activate(p, p->perm[e++]);
  }
  return p->score[p->tree[p->ntree - 1]];
}

/* bruteforcechainingscores for global ov */
static void bruteforce(Problem *p)
{
  uint64_t i, j;

  for (i = 0; i < p->n; i++)
  {
    vsa_chbest b;
    memset(&b, 0, sizeof b);
    for (j = 0; j < i; j++)
    {
      vsa_chcand c;
      candidate(p, (uint32_t) j, &c);
      vsa_ch_fold(p->r, &b, &c, (uint32_t) j, p->f + i);
    }
    vsa_ch_settle(p->r, &b, p->f + i, (uint32_t) i, p->score + i, p->prev + i,
                  p->first + i);
  }
}

static int rightmax(const Problem *p, uint64_t i)
{
  const int last = i + 1 == p->n;
  return vsa_ch_rightmax(last, last ? 0 : p->prev[i + 1],
                         last ? 0 : p->score[i + 1], (uint32_t) i,
                         p->score[i]);
}

static int descending(const void *a, const void *b)
{
  const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
  return x < y ? 1 : x > y ? -1 : 0;
}

/* the chains of one problem through emit(); 0 or a negative code */
typedef struct
{
  uint64_t nchains, nmembers, chaincap, membercap;
  uint64_t *problem, *number, *start, *members;
  int64_t *score;
} Sinkarrays;

static void emit(Sinkarrays *o, const Problem *p, const uint32_t *who,
                 uint64_t problem, uint64_t number, int64_t score,
                 uint32_t end)
{
  uint64_t len = 0, k;
  uint32_t i;

  for (i = end; i != VSA_CHAIN_NONE; i = p->prev[i])
  {
    len++;
  }
  if (o->nchains < o->chaincap)
  {
    if (o->problem != NULL)
    {
      o->problem[o->nchains] = problem;
    }
    if (o->number != NULL)
    {
      o->number[o->nchains] = number;
    }
    if (o->score != NULL)
    {
      o->score[o->nchains] = score;
    }
    if (o->start != NULL)
    {
      o->start[o->nchains] = o->nmembers;
    }
  }
  if (o->members != NULL && o->nmembers + len <= o->membercap)
  {
    for (i = end, k = len; i != VSA_CHAIN_NONE; i = p->prev[i])
    {
      o->members[o->nmembers + --k] = who[i];
    }
  }
  o->nchains++;
  o->nmembers += len;
}

static void chainproblem(Problem *p, const uint32_t *who, uint64_t problem,
                         Sinkarrays *o)
{
  const int kind = p->r->kind, local = vsa_ch_islocal(kind);
  uint64_t i, number = 0, nkeys = 0;
  int64_t best = 0, top = 0, kth = 0, minscore;
  int defined = 0;

  if (p->n == 1)
  {
    p->prev[0] = VSA_CHAIN_NONE;
    emit(o, p, who, problem, 0, vsa_ch_single(kind, p->f), 0);
    return;
  }
  if (kind == VSA_CHAIN_GLOBAL_OV)
  {
    bruteforce(p);
  } else
  {
    top = sweep(p);
  }
  /* retrievemaximalscore, determineequivreps, retrievechainbestscores */
  for (i = 0; i < p->n; i++)
  {
    p->avail[i] = 0;
  }
  for (i = 0; i < p->n; i++)
  {
    if (rightmax(p, i))
    {
      const int64_t s = vsa_ch_endscore(kind, p->score[i], p->tg[i]);
      const uint32_t c = p->first[i];
      if (!defined || best < s)
      {
        best = s;
        defined = 1;
      }
      if (local && (!p->avail[c] || p->cbest[c] < p->score[i]))
      {
        p->cbest[c] = p->score[i];
        p->avail[c] = 1;
      }
      p->key[nkeys++] = (uint64_t) p->score[i];
    }
  }
  if (kind == VSA_CHAIN_LOCAL_BEST)
  {
    /* dictmaxsize.c keeps the value largest distinct keys, as unsigned */
    uint64_t distinct = 0;
    qsort(p->key, (size_t) nkeys, sizeof *p->key, descending);
    for (i = 0; i < nkeys; i++)
    {
      if (i == 0 || p->key[i] != p->key[i - 1])
      {
        kth = (int64_t) p->key[i];
        if (++distinct == (uint64_t) p->r->value)
        {
          break;
        }
      }
    }
  }
  minscore = vsa_ch_threshold(p->r, kind == VSA_CHAIN_GLOBAL ? top : best,
                              kth);
  /* retrievechainthreshold */
  for (i = 0; i < p->n; i++)
  {
    if (rightmax(p, i))
    {
      const int64_t s = vsa_ch_endscore(kind, p->score[i], p->tg[i]);
      if (s < minscore)
      {
        continue;
      }
      if (local)
      {
        const uint32_t c = p->first[i];
        if (!p->avail[c] || p->cbest[c] != s)
        {
          continue;
        }
        p->avail[c] = 0;
      }
      emit(o, p, who, problem, number++, s, (uint32_t) i);
    }
  }
}

/* ---- the whole list --------------------------------------------------------- */

int vsa_chain_host(const vsa_sinkparams *layout,
                   const vsa_chainparams *params, const vsa_match *matches,
                   const uint8_t *palindromic, uint64_t n,
                   vsa_chainstats *stats, uint64_t *problem, uint64_t *number,
                   int64_t *score, uint64_t *start, uint64_t chaincapacity,
                   uint64_t *members, uint64_t membercapacity)
{
  static const char who[] = "vsa_chain_host";
  vsa_selrules view;
  vsa_clrules seqs;
  vsa_chainstats st;
  Sinkarrays out = {0, 0, chaincapacity, membercapacity, problem, number,
                    start, members, score};
  Problem p;
  vsa_chfrag *frag = NULL, *pf = NULL;
  uint64_t *seq1 = NULL, *seq2 = NULL, *key = NULL;
  uint32_t *order = NULL, *tmp = NULL, *rank = NULL;
  uint64_t i, first, runsize = 0, nproblems = 0;
  int onepair = 1, grouped, runtie = 0;
  int rc = vsa_ch_checklayout(layout, params, who, &view, &seqs);

  if (rc != 0 || (rc = vsa_list_check(who, "records", matches, n)) != 0)
  {
    return rc;
  }
  memset(&st, 0, sizeof st);
  memset(&p, 0, sizeof p);
  st.matches = n;
  frag = malloc((size_t) (n + 1) * sizeof *frag);
  pf = malloc((size_t) (n + 1) * sizeof *pf);
  seq1 = malloc((size_t) (n + 1) * sizeof *seq1);
  seq2 = malloc((size_t) (n + 1) * sizeof *seq2);
  key = malloc((size_t) (n + 1) * sizeof *key);
  order = malloc((size_t) (n + 1) * sizeof *order);
  tmp = malloc((size_t) (n + 1) * sizeof *tmp);
  rank = malloc((size_t) (n + 1) * sizeof *rank);
  p.tg = malloc((size_t) (n + 1) * sizeof *p.tg);
  p.score = malloc((size_t) (n + 1) * sizeof *p.score);
  p.cbest = malloc((size_t) (n + 1) * sizeof *p.cbest);
  p.prev = malloc((size_t) (n + 1) * sizeof *p.prev);
  p.first = malloc((size_t) (n + 1) * sizeof *p.first);
  p.perm = malloc((size_t) (n + 1) * sizeof *p.perm);
  p.tree = malloc((size_t) (n + 1) * sizeof *p.tree);
  p.key = malloc((size_t) (n + 1) * sizeof *p.key);
  p.avail = malloc((size_t) n + 1);
  if (frag == NULL || pf == NULL || seq1 == NULL || seq2 == NULL ||
      key == NULL || order == NULL || tmp == NULL || rank == NULL ||
      p.tg == NULL || p.score == NULL || p.cbest == NULL || p.prev == NULL ||
      p.first == NULL || p.perm == NULL || p.tree == NULL || p.key == NULL ||
      p.avail == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  p.r = params;
  p.tmp = tmp;
  for (i = 0; i < n; i++)
  {
    int pal;
    if ((rc = vsa_list_flag(who, layout->kind, palindromic, i, &pal)) != 0)
    {
      goto done;
    }
    if (vsa_ch_view(&view, &seqs, params->weightfactor, matches + i, pal,
                    frag + i, seq1 + i, seq2 + i) != 0)
    {
      rc = vsa_list_misfit(who, i);
      goto done;
    }
    if (seq1[i] != seq1[0] || seq2[i] != seq2[0])
    {
      onepair = 0;
    }
    order[i] = (uint32_t) i;
  }
  /* vmatchchaining, chainvm.c:471-497 */
  grouped = params->withinborders && !onepair;
  if (grouped)
  {
    if ((rc = vsa_ch_grouprank(seq1, seq2, order, n, rank)) != 0)
    {
      goto done;
    }
    for (i = 0; i < n; i++)
    {
      order[rank[i]] = (uint32_t) i;
    }
  }
  for (first = 0, i = 1; i <= n; i++)
  {
    uint64_t size, k, big0 = 0, big1 = 0;
    uint32_t *who = order + first;
    int tie = 0;
    if (i < n && (!grouped || (seq1[order[i]] == seq1[order[i - 1]] &&
                               seq2[order[i]] == seq2[order[i - 1]])))
    {
      continue;
    }
    size = i - first;
    /* possiblysortvmatchmatches: glibc's merging qsort by position2 */
    for (k = 0; k < size; k++)
    {
      key[who[k]] = frag[who[k]].s1;
    }
    sortidx(who, tmp, size, key);
    for (k = 0; k < size; k++)
    {
      pf[k] = frag[who[k]];
      big0 = pf[k].e0 > big0 ? pf[k].e0 : big0;
      big1 = pf[k].e1 > big1 ? pf[k].e1 : big1;
      if (k > 0 && pf[k].s1 == pf[k - 1].s1)
      {
        tie = 1;
        if (k < 2 || pf[k - 2].s1 != pf[k].s1)
        {
          st.tieruns++;
        }
      }
    }
    for (k = 0; k < size; k++)
    {
      p.tg[k] = vsa_ch_terminalgap(params->kind, big0, big1, pf[k].e0,
                                   pf[k].e1);
    }
    p.n = size;
    p.f = pf;
    chainproblem(&p, who, nproblems, &out);
    nproblems++;
    switch (vsa_ch_classof(size, VSA_CH_SMALLMAX, VSA_CH_WAVEMAX))
    {
      case VSA_CH_SINGLE:
        st.single++;
        break;
      case VSA_CH_SMALL:
        st.small++;
        break;
      case VSA_CH_WAVE:
        st.wave++;
        break;
      default:
        st.group++;
    }
    st.largest = size > st.largest ? size : st.largest;
    /* the run of one seqnum1 ends here? */
    runsize += size;
    runtie |= tie;
    if (i == n || seq1[order[i]] != seq1[order[i - 1]])
    {
      if (grouped && runtie && runsize > VSA_CH_STABLEWIDTH)
      {
        st.replayed += runsize;
      }
      runsize = 0;
      runtie = 0;
    }
    first = i;
  }
  st.problems = nproblems;
  st.chains = out.nchains;
  st.chained = out.nmembers;
  if (stats != NULL)
  {
    *stats = st;
  }
  if (start != NULL && out.nchains <= chaincapacity)
  {
    start[out.nchains] = out.nmembers;
  }
  if (((problem != NULL || number != NULL || score != NULL ||
        start != NULL) && out.nchains > chaincapacity) ||
      (members != NULL && out.nmembers > membercapacity))
  {
    rc = vsa_fail(-3, "%s: %lu chains of %lu members, room for %lu and %lu",
                  who, (unsigned long) out.nchains,
                  (unsigned long) out.nmembers, (unsigned long) chaincapacity,
                  (unsigned long) membercapacity);
  }
done:
  free(frag);
  free(pf);
  free(seq1);
  free(seq2);
  free(key);
  free(order);
  free(tmp);
  free(rank);
  free(p.tg);
  free(p.score);
  free(p.cbest);
  free(p.prev);
  free(p.first);
  free(p.perm);
  free(p.tree);
  free(p.key);
  free(p.avail);
  return rc;
}
