/*
  The rules of the sequence clustering, stated ONCE for the host
  (cluster_host.c) and for the kernels (cluster.hip): which records of a match
  list vmatch -dbcluster percsmall perclarge turns into edges between the
  sequences of the index (Vmatch/vmcluster.c:289-295,358-415, the mirror-image
  rule of Vmatch/procfinal.c:159-167, findboundaries of
  kurtz-basic/multiseq.c).  Plain C that both compilers read; all arithmetic
  is 64-bit unsigned.
*/
#ifndef VSA_CLUSTER_RULES_H
#define VSA_CLUSTER_RULES_H
#include <stdint.h>
#include "vstree_amd.h"

#ifdef __HIPCC__
#define VSA_CLHD __host__ __device__ static inline
#else
#define VSA_CLHD static inline
#endif

/* what becomes of a record */
#define VSA_CL_EDGE 0     /* an edge (seq1, seq2)                           */
#define VSA_CL_BAD 1      /* it does not fit the layout                     */
#define VSA_CL_SAME 2     /* seq1 == seq2 (vmcluster.c:368)                 */
#define VSA_CL_MIRROR 3   /* palindromic list, seq1 > seq2                  */
#define VSA_CL_REJECTED 4 /* the overlap is too small                       */
#define VSA_CL_CLASSES 5

typedef struct
{
  uint64_t totallength, numofsequences;
  const uint64_t *markpos; /* numofsequences - 1 separator positions        */
  uint64_t percsmall, perclarge;
} vsa_clrules;

/* sequence s occupies [*start, *end) */
VSA_CLHD void vsa_cl_bounds(const vsa_clrules *r, uint64_t s, uint64_t *start,
                            uint64_t *end)
{
  *start = s == 0 ? 0 : r->markpos[s - 1] + 1;
  *end = s + 1 == r->numofsequences ? r->totallength : r->markpos[s];
}

/* the sequence [pos, pos + length) lies in: the number of separators below
   pos; -1 if the interval is empty, touches a separator or leaves the text */
VSA_CLHD int vsa_cl_seqof(const vsa_clrules *r, uint64_t pos, uint64_t length,
                          uint64_t *seq)
{
  uint64_t lo = 0, hi = r->numofsequences - 1, start, end;

  if (length == 0 || pos >= r->totallength || length > r->totallength - pos)
  {
    return -1;
  }
  while (lo < hi)
  {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (r->markpos[mid] < pos)
    {
      lo = mid + 1;
    } else
    {
      hi = mid;
    }
  }
  vsa_cl_bounds(r, lo, &start, &end);
  if (pos < start || pos + length > end)
  {
    return -1;
  }
  *seq = lo;
  return 0;
}

/* sufficientoverlap, vmcluster.c:289-295 */
VSA_CLHD int vsa_cl_sufficient(uint64_t matchlength, uint64_t seqlen,
                               uint64_t percentage)
{
  return matchlength >= seqlen * percentage / 100;
}

/* A record of a self list (palindromic == 0: length, start1, start2
   absolute, 0) or of a list of vmatch -p IDX (palindromic != 0: dbstart
   absolute, queryseq = the sequence of the index whose reverse complement
   matched, querystart = the offset in that reverse complement) -> VSA_CL_...;
   seq1 and seq2 are set unless the answer is VSA_CL_BAD.  length1 == length2
   for every record of these lists. */
VSA_CLHD int vsa_cl_classify(const vsa_clrules *r, const vsa_match *m,
                             int palindromic, uint64_t *seq1, uint64_t *seq2)
{
  uint64_t s1, e1, s2, e2, small, large;

  if (vsa_cl_seqof(r, m->dbstart, m->length, seq1) != 0)
  {
    return VSA_CL_BAD;
  }
  if (palindromic)
  {
    if (m->queryseq >= r->numofsequences)
    {
      return VSA_CL_BAD;
    }
    *seq2 = m->queryseq;
    vsa_cl_bounds(r, *seq2, &s2, &e2);
    if (m->querystart > e2 - s2 || m->length > e2 - s2 - m->querystart)
    {
      return VSA_CL_BAD;
    }
  } else
  {
    if (vsa_cl_seqof(r, m->queryseq, m->length, seq2) != 0)
    {
      return VSA_CL_BAD;
    }
    vsa_cl_bounds(r, *seq2, &s2, &e2);
  }
  if (*seq1 == *seq2)
  {
    return VSA_CL_SAME;
  }
  if (palindromic && *seq1 > *seq2)
  {
    return VSA_CL_MIRROR;
  }
  vsa_cl_bounds(r, *seq1, &s1, &e1);
  small = e1 - s1;
  large = e2 - s2;
  if (small > large)
  {
    const uint64_t t = small;
    small = large;
    large = t;
  }
  return (vsa_cl_sufficient(m->length, small, r->percsmall) &&
          vsa_cl_sufficient(m->length, large, r->perclarge))
             ? VSA_CL_EDGE
             : VSA_CL_REJECTED;
}

/* ---- what cluster.hip needs of cluster_host.c ---------------------------- */
#ifdef __cplusplus
extern "C" {
#endif

/* clusters in output numbering, owned arrays */
typedef struct
{
  uint64_t numofsequences, clusters, inclusters;
  uint64_t *clusterstart; /* clusters + 1                                   */
  uint64_t *members;      /* inclusters                                     */
  uint64_t *label;        /* numofsequences, VSA_CLUSTER_SINGLET            */
} vsa_clresult;

/* 0, or the message and -2 / VSA_NOT_COVERED of vsa_cluster_open */
int vsa_cl_checklayout(const vsa_sinkparams *layout,
                       const vsa_clusterparams *params, const char *who);
/* the edges (e1[i], e2[i]) in this order through linkcluster; *changed = the
   number of them that joined two different clusters */
int vsa_cl_replay(uint64_t numofsequences, const uint32_t *e1,
                  const uint32_t *e2, uint64_t nedges, uint64_t *changed,
                  vsa_clresult *result);
void vsa_cl_freeresult(vsa_clresult *result);
int64_t vsa_cl_format(const vsa_clresult *result, char *buffer,
                      uint64_t capacity);

#ifdef __cplusplus
}
#endif

#endif
