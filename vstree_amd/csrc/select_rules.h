/*
  The rules of the match selection, stated ONCE for the host (select_host.c)
  and for the kernels (select.hip): what processfinal derives from a match
  (Vmatch/procfinal.c:408-497, 195-257), what matchokay lets through
  (Vmatch/mokay.c:7-114) and the order of the best-match list
  (kurtz/bestmatch.c:33-119).  Plain C that both compilers read; every double
  operation is a multiplication or one division, in the reference's order,
  so host and device agree bit for bit.
*/
#ifndef VSA_SELECT_RULES_H
#define VSA_SELECT_RULES_H
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"
#include "evalues.h"

#ifdef __HIPCC__
#define VSA_HD __host__ __device__ static inline
#else
#define VSA_HD static inline
#endif

#define VSA_SELECT_KEYWORDS 5

typedef struct
{
  int kind;              /* VSA_SINK_...                                   */
  int noevalue;          /* VSA_SHOW_NOEVALUE: every E-value is 0.0        */
  int hasindexedqueries; /* self layout on an index with queries           */
  uint64_t leastlength;
  uint64_t dblenplus1;   /* DATABASELENGTH + 1, subtracted from position2
                            of such a self match (procfinal.c:466-474)     */
  double totallength;    /* (double) totallength: -q multiplier            */
  double multiplier;     /* complete and self layouts                      */
  /* the query Multiseq: sequence q = queryseq - seqoffset starts at
     qstart[q] and has qlen[q] symbols; uniformlen != 0: every sequence has
     that length and starts at q * (uniformlen + 1), no arrays */
  uint64_t nq, seqoffset;
  uint32_t uniformlen;
  const uint64_t *qstart, *qlen;
  /* T with its line starts (lines 0 .. nlines - 1; linestart has nlines + 1
     entries) and hequot[0 .. nlines - 1] */
  const double *table;
  const int64_t *linestart;
  const double *hequot;
  int64_t nlines;
  /* matchokay */
  int hasmaxevalue;
  double maximumevalue;
  uint32_t identity;
  int hasleastscore;
  int64_t leastscore;
  int haslowergap, hasuppergap;
  int64_t lowergap, uppergap;
  /* the selection is full: a key not below its worst one cannot enter */
  int hasworst;
  uint64_t worst[VSA_SELECT_KEYWORDS];
} vsa_selrules;

typedef struct
{
  uint64_t length1, position1, length2, position2;
  int64_t distance;
  double evalue;
} vsa_selvalues;

/* inclookupEvalue (kurtz/evalues.c:370-386); a length the line does not
   reach from below (length <= distance) reads 0.0 */
VSA_HD double vsa_sel_lookup(const vsa_selrules *r, int64_t distance,
                             uint64_t length)
{
  int64_t i;

  if (distance >= r->nlines || length <= (uint64_t) distance ||
      length > (uint64_t) 1 << 40)
  {
    return 0.0;
  }
  i = r->linestart[distance] + (int64_t) length;
  if (i < r->linestart[distance + 1] + distance + 2)
  {
    return r->table[i];
  }
  return 0.0;
}

/* what processfinal derives; 0, or -1 for a record that does not fit the
   layout (a query number outside the batch, a match that leaves its
   sequence) */
VSA_HD int vsa_sel_values(const vsa_selrules *r, const vsa_match *m,
                          int palindromic, vsa_selvalues *v)
{
  double multiplier, t;
  uint64_t lenmatch;
  int64_t ad;
  const int iscomplete = r->kind == VSA_SINK_COMPLETE ||
                         r->kind == VSA_SINK_APPROX_EDIST ||
                         r->kind == VSA_SINK_APPROX_HAMMING;

  v->position1 = m->dbstart;
  v->length1 = m->length;
  v->distance = 0;
  if (r->kind == VSA_SINK_SELF)
  {
    /* convertthematch, Vmatch/procfinal.c:450-475 */
    v->length2 = m->length;
    v->position2 = m->queryseq;
    if (r->hasindexedqueries)
    {
      if (m->queryseq < r->dblenplus1)
      {
        return -1;
      }
      v->position2 -= r->dblenplus1;
    }
    multiplier = r->multiplier;
  } else
  {
    const uint64_t q = m->queryseq - r->seqoffset;
    uint64_t seqstart2, seqlength2, relpos2;
    if (m->queryseq < r->seqoffset || q >= r->nq)
    {
      return -1;
    }
    if (r->uniformlen != 0)
    {
      seqlength2 = r->uniformlen;
      seqstart2 = q * ((uint64_t) r->uniformlen + 1);
    } else
    {
      seqlength2 = r->qlen[q];
      seqstart2 = r->qstart[q];
    }
    if (r->kind == VSA_SINK_QUERY)
    {
      v->length2 = m->length;
      relpos2 = m->querystart;
      multiplier = r->totallength * (double) seqlength2;
    } else
    {
      /* initcompletematchstruct, Vmengine/initcompl.c:7-21 */
      v->length2 = seqlength2;
      relpos2 = 0;
      if (r->kind == VSA_SINK_APPROX_EDIST)
      {
        v->distance = (int64_t) m->querystart;
      } else if (r->kind == VSA_SINK_APPROX_HAMMING)
      {
        v->distance = -(int64_t) m->querystart;
      }
      multiplier = r->multiplier;
    }
    if (relpos2 > seqlength2 || v->length2 > seqlength2 - relpos2)
    {
      return -1;
    }
    if (palindromic)
    {
      relpos2 = seqlength2 - (relpos2 + v->length2); /* procfinal.c:152-158 */
    }
    v->position2 = seqstart2 + relpos2;
  }
  /* assignEvalue, Vmatch/procfinal.c:195-257; incgetEvalue,
     kurtz/evalues.c:388-426 */
  ad = v->distance < 0 ? -v->distance : v->distance;
  lenmatch = (iscomplete || v->distance == 0)
                 ? v->length2
                 : (v->length1 > v->length2 ? v->length1 : v->length2);
  if (r->noevalue || v->distance > VSA_EVALUES_MAXEDIST || ad >= r->nlines)
  {
    v->evalue = 0.0;
  } else
  {
    t = vsa_sel_lookup(r, ad, lenmatch);
    if (v->distance <= 0)
    {
      v->evalue = multiplier * t;
    } else
    {
      const double mh = multiplier * r->hequot[ad];
      v->evalue = mh * t;
    }
  }
  return 0;
}

/* EVALDISTANCE2SCORE, include/match.h:114-116 */
VSA_HD int64_t vsa_sel_score(const vsa_selvalues *v)
{
  const int64_t both = (int64_t) (v->length1 + v->length2);
  return v->distance >= 0 ? both - 3 * v->distance
                          : -(both + 3 * v->distance);
}

/* EVALIDENTITY, include/match.h:122-135 */
VSA_HD double vsa_sel_identity(const vsa_selvalues *v)
{
  const int64_t ad = v->distance < 0 ? -v->distance : v->distance;
  const uint64_t longer = v->length1 > v->length2 ? v->length1 : v->length2;
  const double quot = (double) ad / (double) longer;
  const double rest = 1.0 - quot;
  return 100.0 * rest;
}

/* matchokay, Vmatch/mokay.c:7-114 */
VSA_HD int vsa_sel_okay(const vsa_selrules *r, const vsa_selvalues *v)
{
  if (v->length1 < r->leastlength || v->length2 < r->leastlength)
  {
    return 0;
  }
  if (r->identity > 0 && vsa_sel_identity(v) < (double) r->identity)
  {
    return 0;
  }
  if (r->hasleastscore && vsa_sel_score(v) < r->leastscore)
  {
    return 0;
  }
  if (r->hasmaxevalue && v->evalue > r->maximumevalue)
  {
    return 0;
  }
  if (r->haslowergap)
  {
    int64_t gap;
    if (v->position1 + v->length1 - 1 > v->position2)
    {
      gap = -(int64_t) (v->position1 + v->length1 - v->position2);
    } else
    {
      gap = (int64_t) (v->position2 - (v->position1 + v->length1));
    }
    if (gap < r->lowergap || (r->hasuppergap && gap > r->uppergap))
    {
      return 0;
    }
  }
  return 1;
}

/* cmpBestMatch (kurtz/bestmatch.c:33-119) as five words that compare like
   unsigned numbers, the best match first: an E-value is never negative, so
   its bit pattern orders like the value */
VSA_HD void vsa_sel_key(const vsa_selvalues *v, int palindromic,
                        uint64_t key[VSA_SELECT_KEYWORDS])
{
  uint64_t bits;
  const double e = v->evalue;

  memcpy(&bits, &e, 8);
  key[0] = bits;
  key[1] = ~v->length1;
  key[2] = v->position1;
  key[3] = ~v->length2;
  key[4] = v->position2 << 1 | (palindromic ? 1u : 0u);
}

VSA_HD int vsa_sel_keycmp(const uint64_t *a, const uint64_t *b)
{
  int w;
  for (w = 0; w < VSA_SELECT_KEYWORDS; w++)
  {
    if (a[w] != b[w])
    {
      return a[w] < b[w] ? -1 : 1;
    }
  }
  return 0;
}

#endif
