/*
  Degenerate matches by edit distance, vmatch -l L -e K [-seedlength S] [-p]
  [-q Q] IDX: the entries.  Included by vstree_amd.h, which holds the record
  layout (VSA_EDIST_*), the sink kinds (VSA_SINK_QUERY_EDIST, _SELF_EDIST) and
  VSA_EXTEND_EDIST_MAXDIST; a header of its own as the multi-GPU entries have
  one, so that the list of entries of vstree_amd.h stays what it was.

  What the reference does: the seed length is max(S, L / (K + 1))
  (Vmatch/matchlenparm.c:11-22; vsa_extend_seedlength); the seeds are the
  MEMs of that length in the order of findquerymatches or, without -q, the
  maximal repeats in the order of findselfmatches, as for -h K; every seed on
  its own goes through editextend (kurtz/extendED.c:78-355): a greedy front
  of at most K edit operations to the left and one to the right
  (extendedleftSEP, extendedrightSEP, kurtz/frontSEP.c:192-339), then every
  pair of a left and a right front entry is a candidate, and the best one of
  at least L symbols in both instances is kept -- best by E-value, then
  identity, then length, the later candidate on a tie (include/extcmp.c).
  Self matches also pass acceptmatch (extendED.c:24-48).
*/
#ifndef VSTREE_AMD_EDIST_H
#define VSTREE_AMD_EDIST_H
#include "vstree_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* VSA_EXTEND_EDIST_MAXDIST */
uint32_t vsa_extend_edist_maxdist(void);

/*
  editextend for every seed of a list in HBM; arguments, order of the result
  and the meaning of palindromic as for vsa_extend_hamming.  Every front of a
  side is made by a group of 16, 32 or 64 lanes (2 K + 1 diagonals); a slide
  along equal symbols that has not ended after VSA_EXTEND_LANE_BUDGET symbols
  is finished by the lanes of the group together.  VSA_EXTEND_STAGE in the
  environment forces one form for every slide (`lane`, `long`); the lists are
  the same.  The fronts are kept in device scratch, 8 (K + 1)^2 bytes per
  seed, so the list is worked through in pieces that fit a fixed budget
  (VSA_EXTEND_EDIST_SCRATCH in the environment: that many bytes instead).
  Stats of the result: count = matches, sumlength = sum of length1,
  candidates = seeds, searches = sides with a slide the group finished,
  search_kernel_ms = HIP-event time of fronts and choice (first_kernel_ms =
  of the fronts alone), total_device_ms = of the whole call.
  VSA_NOT_COVERED, nothing delivered, no device memory kept: K above
  VSA_EXTEND_EDIST_MAXDIST, a text or query sequence of 2^32 - 16 symbols or
  more, 2^31 seeds or more, a packed-pair seed list.
  -2: K = 0, L = 0, a layout of another kind, a seed that does not fit the
  index or its query sequence (nothing is read through such a seed).
*/
int vsa_extend_edist(const vsa_index *index, const vsa_queries *queries,
                     const vsa_result *seeds, const vsa_sinkparams *layout,
                     int palindromic, uint64_t leastlength, uint64_t maxdist,
                     uint64_t seedlength, vsa_result **result);

/* vmatch -l L -e K [-seedlength S] [-p] -q Q IDX: the seed length rule,
   vsa_findquerymatches, vsa_extend_edist; errors as for
   vsa_findquerymatches_hamming */
int vsa_findquerymatches_edist(const vsa_index *index,
                               const vsa_queries *queries,
                               uint64_t leastlength, uint64_t maxdist,
                               uint64_t seedlength, int palindromic,
                               vsa_result **result);
/* vmatch -l L -e K [-seedlength S] IDX: the same with
   vsa_findmaximalrepeats */
int vsa_findselfmatches_edist(const vsa_index *index, uint64_t leastlength,
                              uint64_t maxdist, uint64_t seedlength,
                              vsa_result **result);

/*
  The same extension on the host, arguments as for vsa_extend_hamming_host;
  any K up to VSA_EDIST_MAXDISTANCE.  -2 with "record %lu does not fit the
  layout" for a seed outside the index or its query sequence.
  VSA_EXTEND_EDIST_SCALAR in the environment: the slides look at one symbol
  at a time instead of eight (the lists are the same).
*/
int vsa_extend_edist_host(const vsa_sinkparams *layout, const uint8_t *text,
                          const uint8_t *querysymbols, const vsa_match *seeds,
                          uint64_t numofseeds, uint64_t leastlength,
                          uint64_t maxdist, uint64_t seedlength, int threads,
                          vsa_match *matches, uint64_t capacity,
                          uint64_t *numofmatches);

#ifdef __cplusplus
}
#endif
#endif
