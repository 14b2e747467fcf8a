/*
  The rules of the match clustering, stated ONCE for the host
  (matchcluster_host.c) and for the kernels (matchcluster.hip): which pairs of
  matches vmatch -pp matchcluster gapsize G | overlap P links
  (Vmatch/clpos.c:14-201).  Every match m gives the two references
  (position1, 2m) and (position2, 2m + 1) on ONE axis; they are sorted by
  their start alone, equal starts in the order of their index.  Reference i
  then looks at the references j > i of that order until the first one that
  ends its loop; all arithmetic on positions is 64-bit unsigned, as in the
  reference.  What a match is (length1, position1, position2) is the view of
  select_rules.h (vsa_sel_values).  Plain C that both compilers read; the
  overlap is one conversion, one multiplication and one division of doubles,
  so host and device agree bit for bit.
*/
#ifndef VSA_MATCHCLUSTER_RULES_H
#define VSA_MATCHCLUSTER_RULES_H
#include <stdint.h>
#include <string.h>
#include "vstree_amd.h"
#include "select_rules.h"
#include "cluster_rules.h"

/* what becomes of a candidate pair (i, j): the numbers are classes of the
   compaction cluster.hip shares (VSA_CL_CLASSES of them) */
#define VSA_MC_EDGE VSA_CL_EDGE      /* stored                              */
#define VSA_MC_SAME VSA_CL_SAME      /* both references of one match        */
#define VSA_MC_BELOW VSA_CL_REJECTED /* overlap below the threshold         */

/* gap bounds from here on could not be told from a wrapped difference */
#define VSA_MC_MAXGAP ((uint64_t) 1 << 62)

typedef struct
{
  int mode; /* VSA_MATCHCLUSTER_GAP or _OVERLAP */
  uint64_t maxgapsize, minpercentoverlap;
} vsa_mcrules;

/* the loop of reference i over its successors j ends at the first j this
   holds for (clpos.c:91-97 and :149-154) */
VSA_CLHD int vsa_mc_stops(const vsa_mcrules *r, uint64_t end_i,
                          uint64_t start_j)
{
  return r->mode == VSA_MATCHCLUSTER_GAP ? start_j - end_i > r->maxgapsize
                                         : end_i < start_j;
}

/* The same loop as a window of the sorted references, for the kernels.  The
   starts ascend, so in overlap mode the j that do not stop the loop are
   those with start_j <= end_i.  In gap mode either the direct successor
   starts below end_i -- the difference wraps, the loop ends at once
   (vsa_mc_windowempty) -- or every successor starts at end_i or behind it,
   the gaps ascend with j, and the loop runs while start_j <= end_i + G.
   vsa_mc_laststart is that largest start, the sum saturated. */
VSA_CLHD uint64_t vsa_mc_laststart(const vsa_mcrules *r, uint64_t end)
{
  if (r->mode == VSA_MATCHCLUSTER_GAP)
  {
    const uint64_t s = end + r->maxgapsize;
    return s < end ? ~(uint64_t) 0 : s;
  }
  return end;
}

/* the loop of reference i ends at once: its successor starts inside the
   match, and the unsigned gap wraps to a value beyond every bound
   (clpos.c:91-97).  Overlap mode has no such case: start_j >= start_i. */
VSA_CLHD int vsa_mc_windowempty(const vsa_mcrules *r, uint64_t end,
                                uint64_t nextstart)
{
  return r->mode == VSA_MATCHCLUSTER_GAP && nextstart < end;
}

/* a pair inside the window of i -> VSA_MC_...; *value = the gap, or the bits
   of the overlap percentage */
VSA_CLHD int vsa_mc_classify(const vsa_mcrules *r, uint64_t end_i,
                             uint64_t length_i, uint32_t m_i,
                             uint64_t start_j, uint64_t length_j,
                             uint32_t m_j, uint64_t *value)
{
  if (m_i == m_j)
  {
    return VSA_MC_SAME;
  }
  if (r->mode == VSA_MATCHCLUSTER_GAP)
  {
    *value = start_j - end_i;
    return VSA_MC_EDGE;
  } else
  {
    const uint64_t longer = length_i >= length_j ? length_i : length_j;
    const double shared = (double) (end_i - start_j);
    const double scaled = shared * 100.0;
    const double overlap = scaled / (double) longer;
    memcpy(value, &overlap, 8);
    return overlap >= (double) r->minpercentoverlap ? VSA_MC_EDGE
                                                    : VSA_MC_BELOW;
  }
}

/* ---- what matchcluster.hip needs of matchcluster_host.c ------------------ */
#ifdef __cplusplus
extern "C" {
#endif

/* 0, or the message and the code of vsa_matchcluster_open; on success
   *rules describes the view of a match under this layout (host pointers
   into the layout, no E-values) */
int vsa_mc_checklayout(const vsa_sinkparams *layout,
                       const vsa_matchclusterparams *params, const char *who,
                       vsa_selrules *rules, vsa_mcrules *mcrules);
int64_t vsa_mc_format(uint64_t matches, const vsa_clresult *result,
                      char *buffer, uint64_t capacity);

#ifdef __cplusplus
}
#endif

#endif
