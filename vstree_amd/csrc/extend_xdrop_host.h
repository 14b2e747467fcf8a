/* What extend_xdrop.hip asks of extend_xdrop_host.c beside the public entry:
   the seeds whose band outgrew the device, extended by the host rules in
   their places.  Not part of the ABI. */
#ifndef VSA_EXTEND_XDROP_HOST_H
#define VSA_EXTEND_XDROP_HOST_H
#include <stdint.h>
#include "vstree_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* seeds[i] lies at pos2[i] of seq2[0 .. n2), the second Multiseq (self: the
   first one again); seedlength: by the rule already; threads as for the
   public entry.  out[i] and keep[i] for every seed; -101 without memory. */
__attribute__((visibility("hidden")))
int vsa_xd_host_seeds(const uint8_t *seq1, uint64_t n1, const uint8_t *seq2,
                      uint64_t n2, int self, int hamming,
                      const vsa_match *seeds, const uint64_t *pos2,
                      uint64_t numofseeds, uint64_t leastlength,
                      uint64_t xdrop, uint64_t seedlength, int threads,
                      vsa_match *out,
                      uint8_t *keep);

#ifdef __cplusplus
}
#endif
#endif
