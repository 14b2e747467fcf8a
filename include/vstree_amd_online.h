/*
  The scan of the text without an index, vmatch -online -complete [remred]
  [-e K | -h K] -q Q IDX: the entries.  Included by vstree_amd.h; a header of
  its own as the multi-GPU, edit-distance, X-drop and alignment entries have
  one, so that the list of entries of vstree_amd.h stays what it was.

  What the reference does, query by query in the order of the queries
  (decidefcm, Vmengine/fcomplete.c:209-226):
    exact   findexactcompletematchesonline, exactcompl.c:277-325: a
            Boyer-Moore-Horspool scan from left to right; a window matches if
            none of its text symbols is special and all symbols are equal;
            ascending position1.
    -h K    hammingcompletematchesonline, hamcompl.c:9-56, 112-140: start
            positions from n - m down to 0; a window with a separator is no
            match; bytes are compared as they are (a wildcard equals a
            wildcard); distance = -mismatches, length1 = m.
    -e K    findedistcompletematchesonline, edistcompl.c:458-513: the text
            from right to left with the reversed pattern, a separator resets
            the column, every position whose bottom score is <= the
            threshold is a start position (edistmyersbitvectorAPM4 / APM8,
            :261-384, with the Eqsrev masks of kurtz-basic/getEqs.gen up to
            64 symbols: a wildcard equals nothing; edistukkonencutoff,
            :82-172, beyond: bytes as they are).  Every start position goes
            through edistprocessstartpos (approxcompl.c:14-65) with
            maxlength = min(m + k, totallength - start) (edistcompl.c:14-19):
            the best-distance, then longest prefix of longestmatch.c, where a
            wildcard equals nothing for every m, and its distance as it
            comes, above K too.
    remred  CHECKMATCHPOSITION, edistcompl.c:33-80, with -e: of a hit
            directly in front of the stored one the one with the smaller
            score is kept; a hit there that does not improve is dropped and
            ends the run (not "the best of each maximal run").
    Kp      m K / 100 per query (initcompl.c:52-56); with -e a threshold of 0
            still takes the scan of the columns, and nothing refuses a
            threshold >= m.

  Records: those of vsa_findcompletematches for mode 0 and of
  vsa_findapproxcompletematches for modes 1 and 2 -- (length1, dbstart,
  queryseq + offset, distance in the querystart field; the number of
  mismatches for -h) --, so the sink (VSA_SINK_COMPLETE, _APPROX_EDIST,
  _APPROX_HAMMING), vsa_align, selection and coverage take a list found on a
  vsa_index as they take the indexed one.  Order: the order of the queries;
  inside a query ascending dbstart for mode 0, descending for modes 1 and 2.
  -p is a second call on vsa_queries_reverse_complement.
*/
#ifndef VSTREE_AMD_ONLINE_H
#define VSTREE_AMD_ONLINE_H
#include "vstree_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the mapped text alone in one GPU's HBM: what vmatch -online maps, TISTAB
   (Vmatch/mapdemand.c:168-171).  Padded in front and behind as the text of a
   vsa_index is; the padding reads as separators. */
typedef struct vsa_text vsa_text;

int vsa_text_from_host(const uint8_t *tis, uint64_t totallength,
                       uint32_t numofchars, int device, vsa_text **text);
/* totallength symbols in the memory of `device` (copied) */
int vsa_text_from_device(const void *device_tis, uint64_t totallength,
                         uint32_t numofchars, int device, vsa_text **text);
/* NAME.prj and NAME.tis, and NAME.al1 for the number of symbols; no other
   table is looked for */
int vsa_text_open(const char *indexname, int device, vsa_text **text);
void vsa_text_close(vsa_text *text);

/*
  mode 0 exact, 1 -e, 2 -h; distvalue K; percent 0 | 1 as for
  vsa_findapproxcompletematches; removeredundant != 0: -complete remred.
  The text of the index (one with the table bck: from_tables uploads the text
  with it), or a vsa_text, is cut into tiles: an edit scan is a work-item per
  (query, tile) that starts m + k symbols to the right of its tile with a
  reset column; a first pass counts the hits per (query, tile), a second one
  visits only the pairs that have any.  VSA_ONLINE_TILE in the environment,
  read by every call, sets the symbols per tile of the edit scan (a multiple
  of 8 from 64 to the default, VSA_ONLINE_TILE_DEFAULT; a test hook, the
  lists are the same).  The queries are taken in chunks whose (query, tile)
  counters fit a buffer of VSA_ONLINE_COUNTERS_DEFAULT words, and in no more
  than 65535 groups of 32 queries; VSA_ONLINE_COUNTERS in the environment,
  read by every call, sets that number of counters (1 to the default, other
  values are ignored; a test hook as well).  vsa_online_plan() below tells
  how a call is cut.
  Stats of the result: count = matches, sumlength = sum of length1,
  candidates = start positions before remred, searches = (query, tile) pairs
  the second pass visited, search_kernel_ms = HIP-event time of the two
  scans (first_kernel_ms = of the first pass alone), total_device_ms = of
  the whole call.
  All refusals leave nothing delivered and no device memory kept.
  VSA_NOT_COVERED: percent == 2 (Kb: the reference's online min-score scans,
  hamcompl.c:58-110, edistcompl.c:174-259, 386-456, are not restated); mode 1
  on an alphabet other than 4 symbols or with a query of more than 512
  symbols, or with a threshold >= m (every position matches; the host entry
  takes it literally); a query of 2^32 - 16 symbols or more; 2^31 queries or
  more.  Modes 0 and 2 compare bytes and take any alphabet.
  -2: a mode outside 0 .. 2; removeredundant with a mode other than 1 (the
  reference's message, Vmatch/parsevm.c:1448).  -3: an index without bck.
  -1: NULL arguments, queries on another device.
*/
#define VSA_ONLINE_TILE_DEFAULT 296u
#define VSA_ONLINE_COUNTERS_DEFAULT (1ull << 26)
int vsa_findcompletematches_online(const vsa_index *index,
                                   const vsa_queries *queries, int mode,
                                   uint64_t distvalue, int percent,
                                   int removeredundant, vsa_result **result);
int vsa_text_findcompletematches_online(const vsa_text *text,
                                        const vsa_queries *queries, int mode,
                                        uint64_t distvalue, int percent,
                                        int removeredundant,
                                        vsa_result **result);

/*
  A test hook, no GPU needed: how the two entries above cut a text of
  totallength symbols and numofqueries queries, by the function the driver
  itself calls, with VSA_ONLINE_TILE and VSA_ONLINE_COUNTERS as they stand in
  the environment.  *tile: symbols per tile of the edit scan (mode 1), start
  positions per tile of the window scans (modes 0 and 2, 2048); *ntiles:
  tiles of the text, 0 for an empty one (an edit scan launches
  ceil(ntiles / 128) workgroups per group of 32 queries, a window scan
  ntiles); *queries_per_chunk: counters / ntiles, at least 1 and at most
  65535 * 32; *numofchunks: 0 for an empty text or an empty batch.
  -2: a mode outside 0 .. 2.  -1: NULL arguments.
*/
int vsa_online_plan(uint64_t totallength, uint64_t numofqueries, int mode,
                    uint32_t *tile, uint64_t *ntiles,
                    uint64_t *queries_per_chunk, uint64_t *numofchunks);

/*
  The same on the host by the same rules (online_rules.h): query i is
  querysymbols[querystart[i] .. + querylength[i]); the work is cut by (query,
  slice of the text) over `threads` threads (<= 0: one per processor), an
  edit scan of a slice starting m + k symbols to its right.  Any m, any
  alphabet, any threshold.  -3: more than `capacity` matches.
  VSA_NOT_COVERED: percent == 2.  -2 and -1 as above.
*/
int vsa_findcompletematches_online_host(
    const uint8_t *tis, uint64_t totallength, const uint8_t *querysymbols,
    const uint64_t *querystart, const uint64_t *querylength,
    uint64_t numofqueries, uint64_t seqoffset, int mode, uint64_t distvalue,
    int percent, int removeredundant, int threads, vsa_match *matches,
    uint64_t capacity, uint64_t *numofmatches);

#ifdef __cplusplus
}
#endif
#endif
