/*
  X-drop extension of exact seeds, vmatch -l L -hxdrop X | -exdrop X
  [-seedlength S] [-p] [-q Q] IDX: the entries.  Included by vstree_amd.h,
  which holds the record layout (VSA_XDROP_*), the sink kinds
  (VSA_SINK_QUERY_HXDROP .. VSA_SINK_SELF_EXDROP) and VSA_XDROP_MAXDROP; a
  header of its own as the edit-distance entries have one, so that the list
  of entries of vstree_amd.h stays what it was.

  What the reference does: the seed length is S, or 30 if S is not given
  (Vmatch/matchlenparm.c:40-46; vsa_extend_xdrop_seedlength); the seeds are
  the MEMs of that length in the order of findquerymatches or, without -q,
  the maximal repeats in the order of findselfmatches; every seed on its own
  goes through xdropseedextend (Vmengine/xdropext.c:39-221) with
  xdropbelowscore = -X (-hxdrop) or +X (-exdrop), X = 1 .. 255:
    -hxdrop  evalhammingxdropleft / -right (kurtz/xdrop.c:37-140): match +2,
             mismatch -1, stop when the score is below best - X; the left
             scan rejects the seed when it sees S matches in a row
    -exdrop  evaleditxdropleft / -right (kurtz/xdrop.gen:2-201): the greedy
             generations of Zhang et al. with the same scores and -2 for an
             insertion or deletion
  then the two sides are put together, separators at the ends of the match
  are trimmed, self matches pass acceptmatch, and the match is kept if both
  instances have L symbols (matchokay, Vmatch/mokay.c:16-24).  One match per
  seed at most; nothing is chosen by E-value.
  Not covered: -leastscore, -identity or -evalue as the only filter, -allmax,
  six-frame batches.
*/
#ifndef VSTREE_AMD_XDROP_H
#define VSTREE_AMD_XDROP_H
#include "vstree_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* S, or 30 for S = 0 */
uint64_t vsa_extend_xdrop_seedlength(uint64_t seedlength);

/*
  xdropseedextend for every seed of a list in HBM; seeds, layout, queries,
  palindromic and the order of the result as for vsa_extend_hamming.  xdrop
  X; hamming != 0: -hxdrop, 0: -exdrop.
  -hxdrop: one lane per side of a seed, 8 symbols per step; a side not
  finished after VSA_EXTEND_LANE_BUDGET symbols goes to a wavefront that
  covers VSA_EXTEND_LONG_STEP symbols per step.
  -exdrop: a group of 16, 32 or 64 lanes per side, one lane per diagonal of
  the band of the current generation; a slide along equal symbols that has
  not ended after VSA_EXTEND_LANE_BUDGET symbols is finished by the lanes of
  the group together.  X sets no bound on the band: a side whose band
  outgrows its group is done again by a wider group, and one that outgrows
  the widest (64 lanes, or VSA_EXTEND_XDROP_BAND in the environment: 16 or
  32) is handed over -- its seed is fetched, goes through the rules of
  vsa_extend_xdrop_host on the host, and the record is put back in its place.
  VSA_EXTEND_STAGE in the environment (`lane`, `long`) forces one form of
  every scan / slide; the lists are the same.
  Stats of the result: count = matches, sumlength = sum of length1,
  candidates = seeds, searches = sides the long stage scanned (-hxdrop) /
  slides the group finished (-exdrop), kernel_searches = seeds handed over
  to the host rules, search_kernel_ms = HIP-event time of the extension,
  total_device_ms = of the whole call.
  VSA_NOT_COVERED, nothing delivered, no device memory kept: a text or query
  sequence of 2^32 - 16 symbols or more, 2^31 seeds or more, a packed-pair
  or already extended seed list.
  -2: X = 0, X > VSA_XDROP_MAXDROP, L = 0, a layout of another kind, a seed
  that does not fit the index or its query sequence.
*/
int vsa_extend_xdrop(const vsa_index *index, const vsa_queries *queries,
                     const vsa_result *seeds, const vsa_sinkparams *layout,
                     int palindromic, uint64_t leastlength, uint64_t xdrop,
                     int hamming, uint64_t seedlength, vsa_result **result);

/* vmatch -l L -hxdrop X | -exdrop X [-seedlength S] [-p] -q Q IDX: the seed
   length rule, vsa_findquerymatches, vsa_extend_xdrop */
int vsa_findquerymatches_xdrop(const vsa_index *index,
                               const vsa_queries *queries,
                               uint64_t leastlength, uint64_t xdrop,
                               int hamming, uint64_t seedlength,
                               int palindromic, vsa_result **result);
/* ... without -q: the same with vsa_findmaximalrepeats */
int vsa_findselfmatches_xdrop(const vsa_index *index, uint64_t leastlength,
                              uint64_t xdrop, int hamming,
                              uint64_t seedlength, vsa_result **result);

/*
  The same extension on the host, arguments as for vsa_extend_hamming_host
  with xdrop and hamming as above; any band.  VSA_NOT_COVERED: a text or a
  query sequence of 2^32 - 16 symbols or more.  -2 with "record %lu does not
  fit the layout" for a seed outside the index or its query sequence.
  VSA_EXTEND_XDROP_SCALAR in the environment: scans and slides look at one
  symbol at a time instead of eight (the lists are the same).
*/
int vsa_extend_xdrop_host(const vsa_sinkparams *layout, const uint8_t *text,
                          const uint8_t *querysymbols, const vsa_match *seeds,
                          uint64_t numofseeds, uint64_t leastlength,
                          uint64_t xdrop, int hamming, uint64_t seedlength,
                          int threads, vsa_match *matches, uint64_t capacity,
                          uint64_t *numofmatches);

#ifdef __cplusplus
}
#endif
#endif
