/*
  The rules of the chaining, stated ONCE for the host (chain_host.c) and for
  the kernels (chain.hip): what vmatch -pp chain makes of a record
  (vmatchinitfragmentinfo, Vmatch/chainvm.c:29-78), which fragment precedes
  which and with what score (evalfragmentscore and activatefragpoint,
  kurtz-basic/chain2dim.c:990-1148; bruteforcechainingscores, :776-888, for
  global ov), and which chains are retrieved (:1150-1360,1545-1657).

  The reference sweeps over the start and end points in dimension 1 and keeps
  the active fragments in a red-black tree with the key (end0, number).  Its
  answer does not depend on the order of events: the predecessor of fragment
  i is, among the fragments j with end1[j] < start1[i] (active) and
  end0[j] <= start0[i] - 1 (key), the one of greatest priority, and among
  equal priorities the one with the smallest (end1[j], j) -- the one that was
  activated first, which the later ones do not replace (an entry is inserted
  only with a priority strictly above that of its predecessor-or-equal).
  maxgap is asked of that one fragment only.  vsa_ch_fold folds one candidate
  into the best so far, vsa_ch_settle turns the best into score, previous and
  first of the chain; the host's sweep finds j in its tree and settles it
  with the same function.

  A view of a record is that of select_rules.h (lengths, positions,
  distance) with the sequence numbers of cluster_rules.h.  Scores are
  int64_t, positions uint64_t.  The two expressions on doubles (weight,
  percent) are single operations in the reference's order, so host and device
  agree bit for bit.
*/
#ifndef VSA_CHAIN_RULES_H
#define VSA_CHAIN_RULES_H
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"
#include "select_rules.h"
#include "cluster_rules.h"

#define VSA_CHD VSA_CLHD

/* the classes of problems by their number of fragments: one kernel each.
   The two bounds were measured against their neighbours
   (scripts/chain_probe.py --bounds, profiles/r10/README.md) */
#define VSA_CH_SINGLE 0 /* 1 fragment: chainingboundarycases              */
#define VSA_CH_SMALL 1  /* 2 .. VSA_CH_SMALLMAX: one lane per problem     */
#define VSA_CH_WAVE 2   /* .. VSA_CH_WAVEMAX: one wavefront per problem   */
#define VSA_CH_GROUP 3  /* .. VSA_CHAIN_MAXGROUP: one workgroup           */
#define VSA_CH_CLASSES 4
#define VSA_CH_SMALLMAX 8u
#define VSA_CH_WAVEMAX 64u
/* the run of one seqnum1 the reference's quicksort sorts by insertion, which
   keeps the order of equal keys (include/qsort.gen) */
#define VSA_CH_STABLEWIDTH 10u

typedef struct
{
  uint64_t s0, e0, s1, e1; /* inclusive ends                                */
  int64_t w;
} vsa_chfrag;

/* a fragment whose score is final, as a candidate for those behind it */
typedef struct
{
  uint64_t s0, e0, s1, e1;
  int64_t score, tg; /* tg: its terminal gap, 0 for plain global            */
  uint32_t first;
} vsa_chcand;

/* the best candidate so far */
typedef struct
{
  int has, link;  /* link (ov): the candidate continues the chain of j       */
  int64_t key;    /* its priority; ov: the score fragment i would get        */
  int64_t score;  /* of j                                                    */
  uint64_t e0, e1;
  uint32_t j, first;
} vsa_chbest;

VSA_CHD int vsa_ch_classof(uint64_t size, uint32_t smallmax, uint32_t wavemax)
{
  return size <= 1 ? VSA_CH_SINGLE
                   : size <= smallmax
                         ? VSA_CH_SMALL
                         : size <= wavemax ? VSA_CH_WAVE : VSA_CH_GROUP;
}

VSA_CHD int vsa_ch_islocal(int kind)
{
  return kind >= VSA_CHAIN_LOCAL_MAX;
}

/* every kind but plain global has the gap terms (chainvm.c:264-266) */
VSA_CHD int vsa_ch_addterminal(int kind)
{
  return kind != VSA_CHAIN_GLOBAL;
}

/* (Sint) (weightfactor * (double) ABS(DISTANCE2SCORE)), chainvm.c:63-64 */
VSA_CHD int64_t vsa_ch_weight(double weightfactor, const vsa_selvalues *v)
{
  const int64_t score = vsa_sel_score(v);
  const double a = (double) (score < 0 ? -score : score);
  const double scaled = weightfactor * a;
  return (int64_t) scaled;
}

VSA_CHD void vsa_ch_fragment(double weightfactor, const vsa_selvalues *v,
                             vsa_chfrag *f)
{
  f->s0 = v->position1;
  f->e0 = v->position1 + v->length1 - 1;
  f->s1 = v->position2;
  f->e1 = v->position2 + v->length2 - 1;
  f->w = vsa_ch_weight(weightfactor, v);
}

/* chainvm.c:71-75; big0 and big1: the largest ends of the problem */
VSA_CHD int64_t vsa_ch_initialgap(const vsa_chfrag *f)
{
  return (int64_t) (f->s0 + f->s1);
}

VSA_CHD int64_t vsa_ch_terminalgap(int kind, uint64_t big0, uint64_t big1,
                                   uint64_t e0, uint64_t e1)
{
  return vsa_ch_addterminal(kind) ? (int64_t) (big0 - e0 + big1 - e1) : 0;
}

/* evalpriority, chain2dim.c:932-941 (tg is 0 for plain global) */
VSA_CHD int64_t vsa_ch_priority(int64_t score, int64_t tg)
{
  return score - tg;
}

/* fragment j is in the tree when the start of i comes up: at equal
   positions the start goes first (comparestartandend, :1363-1378) */
VSA_CHD int vsa_ch_active(uint64_t e1j, uint64_t s1i)
{
  return e1j < s1i;
}

/* its key is not above (start0[i] - 1, i); none is if start0[i] == 0
   (:1063-1078) */
VSA_CHD int vsa_ch_keyok(uint64_t e0j, uint64_t s0i)
{
  return s0i != 0 && e0j <= s0i - 1;
}

/* candidate a (priority pa, end1 e1a, number a) is taken before b */
VSA_CHD int vsa_ch_beats(int64_t pa, uint64_t e1a, uint32_t a, int64_t pb,
                         uint64_t e1b, uint32_t b)
{
  if (pa != pb)
  {
    return pa > pb;
  }
  if (e1a != e1b)
  {
    return e1a < e1b;
  }
  return a < b;
}

/* checkmaxgapwidth, :740-774 */
VSA_CHD int vsa_ch_maxgapok(uint64_t maxgap, uint64_t e0l, uint64_t e1l,
                            uint64_t s0r, uint64_t s1r)
{
  const uint64_t g0 = s0r <= e0l ? 0 : s0r - e0l - 1,
                 g1 = s1r <= e1l ? 0 : s1r - e1l - 1;
  return g0 <= maxgap && g1 <= maxgap;
}

/* colinearfragments, :147-157 */
VSA_CHD int vsa_ch_colinear(const vsa_chcand *l, const vsa_chfrag *r)
{
  return l->s0 < r->s0 && l->e0 < r->e0 && l->s1 < r->s1 && l->e1 < r->e1;
}

/* overlapcost, :192-217 */
VSA_CHD int64_t vsa_ch_overlap(const vsa_chcand *l, const vsa_chfrag *r)
{
  uint64_t o = 0;
  if (r->s0 <= l->e0)
  {
    o += l->e0 - r->s0 + 1;
  }
  if (r->s1 <= l->e1)
  {
    o += l->e1 - r->s1 + 1;
  }
  return (int64_t) o;
}

/* candidate j (its score final) for fragment i = *f */
VSA_CHD void vsa_ch_fold(const vsa_chainparams *r, vsa_chbest *b,
                         const vsa_chcand *c, uint32_t j, const vsa_chfrag *f)
{
  if (r->kind == VSA_CHAIN_GLOBAL_OV)
  {
    int64_t score;
    int link;
    if ((r->maxgapwidth != 0 &&
         !vsa_ch_maxgapok(r->maxgapwidth, c->e0, c->e1, f->s0, f->s1)) ||
        !vsa_ch_colinear(c, f))
    {
      return;
    }
    score = c->score - vsa_ch_overlap(c, f);
    link = score > 0;
    score = link ? score + f->w : f->w;
    /* the first maximum in the order of the fragments (:855-860) */
    if (!b->has || score > b->key || (score == b->key && j < b->j))
    {
      b->has = 1;
      b->link = link;
      b->key = score;
      b->j = j;
      b->first = c->first;
    }
  } else
  {
    const int64_t p = vsa_ch_priority(c->score, c->tg);
    if (!vsa_ch_active(c->e1, f->s1) || !vsa_ch_keyok(c->e0, f->s0))
    {
      return;
    }
    if (!b->has || vsa_ch_beats(p, c->e1, j, b->key, b->e1, b->j))
    {
      b->has = 1;
      b->link = 1;
      b->key = p;
      b->score = c->score;
      b->e0 = c->e0;
      b->e1 = c->e1;
      b->j = j;
      b->first = c->first;
    }
  }
}

/* evalfragmentscore, :1079-1140, and the end of the loop of
   bruteforcechainingscores, :863-885 */
VSA_CHD void vsa_ch_settle(const vsa_chainparams *r, const vsa_chbest *b,
                           const vsa_chfrag *f, uint32_t i, int64_t *score,
                           uint32_t *prev, uint32_t *first)
{
  int has = b->has;

  *prev = VSA_CHAIN_NONE;
  *first = i;
  if (r->kind == VSA_CHAIN_GLOBAL_OV)
  {
    *score = has ? b->key : f->w;
    if (has && b->link)
    {
      *prev = b->j;
      *first = b->first;
    }
    return;
  }
  if (has && r->maxgapwidth != 0 &&
      !vsa_ch_maxgapok(r->maxgapwidth, b->e0, b->e1, f->s0, f->s1))
  {
    has = 0; /* the second best is not tried (:1083-1090) */
  }
  if (!has)
  {
    *score = f->w - (r->kind == VSA_CHAIN_GLOBAL_GC ? vsa_ch_initialgap(f)
                                                    : 0);
    return;
  }
  if (r->kind == VSA_CHAIN_GLOBAL)
  {
    *score = b->score + f->w;
  } else
  {
    /* gapcostL1, :173-190 */
    const int64_t gc = (int64_t) ((f->s0 - b->e0) + (f->s1 - b->e1));
    if (r->kind != VSA_CHAIN_GLOBAL_GC && !(b->score > gc))
    {
      *score = f->w; /* a new local chain */
      return;
    }
    *score = b->score + (f->w - gc);
  }
  *prev = b->j;
  *first = b->first;
}

/* chainingboundarycases, :251-277: the score of a problem of one fragment */
VSA_CHD int64_t vsa_ch_single(int kind, const vsa_chfrag *f)
{
  /* the fragment holds both largest ends: no terminal gap */
  return f->w - (kind == VSA_CHAIN_GLOBAL_GC ? vsa_ch_initialgap(f) : 0);
}

/* isrightmaximallocalchain, :1150-1167: only fragment i + 1 is looked at */
VSA_CHD int vsa_ch_rightmax(int islast, uint32_t prevnext, int64_t scorenext,
                            uint32_t i, int64_t score)
{
  return islast || prevnext != i || scorenext < score;
}

/* what a chain end is compared with the threshold as, and printed with
   (:1307-1314) */
VSA_CHD int64_t vsa_ch_endscore(int kind, int64_t score, int64_t tg)
{
  return kind == VSA_CHAIN_GLOBAL_GC ? score - tg : score;
}

/* :1613-1615 */
VSA_CHD int64_t vsa_ch_percent(int64_t best, int64_t percent)
{
  const double quot = (double) percent / 100.0;
  const double rest = 1.0 - quot;
  const double scaled = (double) best * rest;
  return (int64_t) scaled;
}

/* the threshold of a problem from the greatest value of its kind: for plain
   global the greatest score of all fragments (the entry with the greatest
   key of the final tree holds it: priorities never fall along the keys, and
   the first fragment of the greatest priority is neither refused nor
   deleted), else the greatest end score of the right-maximal fragments */
VSA_CHD int64_t vsa_ch_threshold(const vsa_chainparams *r, int64_t best,
                                 int64_t kthbest)
{
  switch (r->kind)
  {
    case VSA_CHAIN_LOCAL_THRESHOLD:
      return r->value;
    case VSA_CHAIN_LOCAL_BEST:
      return kthbest;
    case VSA_CHAIN_LOCAL_PERCENT:
      return vsa_ch_percent(best, r->value);
    default:
      return best;
  }
}

/* ---- what chain.hip needs of chain_host.c -------------------------------- */
#ifdef __cplusplus
extern "C" {
#endif

/* 0, or the message and the code of vsa_chain_open; on success the views of
   a record under this layout (host pointers into the layout) */
int vsa_ch_checklayout(const vsa_sinkparams *layout,
                       const vsa_chainparams *params, const char *who,
                       vsa_selrules *rules, vsa_clrules *seqs);
/* groupmatchesbyseqnum (kurtz/matsort.c:316-367) on the n records given in
   any order, entry t with the number recnum[t] and the sequence numbers
   seq1[t] and seq2[t]: rank[t] = the place of entry t in the order the
   stable counting sort by seq1 and the quicksort by seq2 inside every run
   of one seq1 leave */
int vsa_ch_grouprank(const uint64_t *seq1, const uint64_t *seq2,
                     const uint32_t *recnum, uint64_t n, uint32_t *rank);

#ifdef __cplusplus
}
#endif

/* the view of a record: 0, or -1 if it does not fit the layout */
VSA_CHD int vsa_ch_view(const vsa_selrules *view, const vsa_clrules *seqs,
                        double weightfactor, const vsa_match *m,
                        int palindromic, vsa_chfrag *f, uint64_t *seq1,
                        uint64_t *seq2)
{
  vsa_selvalues v;

  if (vsa_sel_values(view, m, palindromic, &v) != 0 || v.length1 == 0 ||
      v.length2 == 0 ||
      vsa_cl_seqof(seqs, v.position1, v.length1, seq1) != 0)
  {
    return -1;
  }
  if (view->kind == VSA_SINK_SELF)
  {
    if (vsa_cl_seqof(seqs, m->queryseq, v.length2, seq2) != 0)
    {
      return -1;
    }
  } else
  {
    *seq2 = m->queryseq - view->seqoffset;
  }
  vsa_ch_fragment(weightfactor, &v, f);
  return 0;
}

#endif
