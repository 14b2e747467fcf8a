/*
  Alignments of degenerate matches, vmatch -s [W]: the edit script of every
  match of a list, and the text vmatch prints for it.  Included by
  vstree_amd.h; a header of its own as the edit-distance entries have one, so
  that the list of entries of vstree_amd.h stays what it was.

  What the reference does (Vmatch/echomatch.c:587-876): a match of distance 0
  gets one identical run (alignequalstrings), a -h match a column by column
  comparison (hammingalignment), a -e match the greedy alignment of its two
  whole substrings (greedyedistalign, kurtz/galign.c:322-420: the fronts of
  kurtz/front.gen with the direction of every entry, then backtracefront);
  showalignment (kurtz/showalign.c) prints the script in blocks of W columns.
  A palindromic match aligns the left substring with the reverse complement
  of the right one.

  A script is a sequence of 16-bit words (include/alignment.h:43-46), LAST
  OPERATION FIRST: a run of up to 16383 identical columns as its length,
  VSA_ALIGN_DELETION (a symbol of the left instance over a gap),
  VSA_ALIGN_INSERTION (a gap over a symbol of the right instance),
  VSA_ALIGN_MISMATCH.  The scripts of a list come in CSR form: the words of
  record i are eops[offsets[i] .. offsets[i + 1]).

  Covered layouts: VSA_SINK_COMPLETE, _QUERY, _SELF, _APPROX_EDIST,
  _APPROX_HAMMING, _QUERY_HAMMING, _SELF_HAMMING, _QUERY_EDIST, _SELF_EDIST.
  VSA_NOT_COVERED: the X-drop kinds (the reference aligns them again with
  another aligner), the translated kinds, selfpalindromic lists.
*/
#ifndef VSTREE_AMD_ALIGN_H
#define VSTREE_AMD_ALIGN_H
#include "vstree_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VSA_ALIGN_MAXRUN 16383u
#define VSA_ALIGN_DELETION 0x4000u
#define VSA_ALIGN_INSERTION 0x8000u
#define VSA_ALIGN_MISMATCH 0xC000u

/* the largest stored distance of the device path: the directions of a
   diagonal over generations 0 .. 31 are the 64 bits of one register */
#define VSA_ALIGN_MAXDIST 31u
uint32_t vsa_align_maxdist(void);

typedef struct vsa_alignments vsa_alignments; /* scripts resident in HBM */

typedef struct
{
  uint64_t count;     /* records                                          */
  uint64_t words;     /* words of all scripts                             */
  uint64_t edist;     /* records aligned by the front kernel              */
  uint64_t staged;    /* ... whose group finished a slide together        */
  double kernel_ms;   /* HIP-event time of the two alignment kernels      */
  double total_device_ms; /* ... of the whole call                        */
} vsa_alignstats;

/*
  The scripts of a match list that stays in HBM.  queries: the forward batch
  the records refer to, NULL for a self layout; of the layout only the kind
  is read; palindromic != 0: the records come from the pass over the reverse
  complement of the batch.  A record of positive distance is aligned by a
  group of 16, 32 or 64 lanes, one lane per diagonal, which keeps the
  directions of its diagonal in a register and runs the backtrace itself;
  the other records by one wavefront each.  VSA_EXTEND_STAGE (`lane`, `long`)
  forces one form of every slide, as for vsa_extend_edist.
  VSA_NOT_COVERED, nothing delivered, no device memory kept: a stored
  distance above VSA_ALIGN_MAXDIST (vsa_align_host takes it), a packed-pair
  result, the kinds and lists named above, texts or query sequences of
  2^32 - 16 symbols or more.
  -2: a record that does not fit its texts or names a match no matcher
  delivers (nothing is read through it), or whose edit distance is above the
  distance it carries.
*/
int vsa_align(const vsa_index *index, const vsa_queries *queries,
              const vsa_result *matches, const vsa_sinkparams *layout,
              int palindromic, vsa_alignments **alignments);
int vsa_alignments_info(const vsa_alignments *alignments,
                        vsa_alignstats *stats);
/* offsets[count + 1] and eops[words] to the host (either may be NULL) */
int vsa_alignments_fetch(const vsa_alignments *alignments, uint64_t *offsets,
                         uint16_t *eops);
void vsa_alignments_free(vsa_alignments *alignments);

/*
  The same scripts on the host, any distance a record can carry.  layout as
  for vsa_extend_hamming_host, with one of the covered kinds; text: the
  symbols of the index; querysymbols: those of the FORWARD batch, also for a
  palindromic list.  offsets[n + 1] is always filled; -3 if the scripts have
  more than `capacity` words (then eops is untouched).  threads 0 = one per
  processor.
*/
int vsa_align_host(const vsa_sinkparams *layout, const uint8_t *text,
                   const uint8_t *querysymbols, const vsa_match *matches,
                   uint64_t n, int palindromic, int threads,
                   uint64_t *offsets, uint16_t *eops, uint64_t capacity);

/*
  For every record the default match line of the sink and, behind it, what
  showalignment prints for its script in blocks of `linewidth` columns (0:
  the reference's 60) -- byte for byte what vmatch -s W prints behind its
  `# args=` line.  origtext / queryorig: the original characters that belong
  to text / querysymbols (IDX.ois, the query file).  Bytes written, or a
  negative code: -3 if the buffer is too small, -2 for a script that does
  not account for the two substrings of its record.
*/
int64_t vsa_align_format(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                         const uint64_t *offsets, const uint16_t *eops,
                         const uint8_t *text, const uint8_t *origtext,
                         const uint8_t *querysymbols,
                         const uint8_t *queryorig, uint32_t linewidth,
                         char *buffer, uint64_t capacity);
/* the same to a FILE * */
int vsa_align_write(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                    const uint64_t *offsets, const uint16_t *eops,
                    const uint8_t *text, const uint8_t *origtext,
                    const uint8_t *querysymbols, const uint8_t *queryorig,
                    uint32_t linewidth, void *file);

#ifdef __cplusplus
}
#endif
#endif
