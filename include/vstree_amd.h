/*
  vstree_amd.h -- C ABI of the MI355X-native Vmengine query path.

  One shared library (vstree_amd/libvstree_amd.so, HIP for gfx950 inside)
  replaces the reference's CPU implementation of

    vmatch -complete -q Q IDX          exact complete matches
    vmatch -l L -q Q IDX               maximal exact matches (MEM)
    vmatch -mum [cand] -l L -q Q IDX   maximal unique matches / candidates
    vmatch -mum -l L IDX               MUMs when the queries are in the index

  on the enhanced suffix array mkvtree writes.  Everything here is plain C:
  pointers, sizes, opaque handles; no HIP or torch types.  Each entry point
  names the reference interface it stands in for (paths relative to
  /root/reference/src); INTEGRATION.md shows the few lines of C a Vmatch
  maintainer adds so that findcompletematches / findquerymatches /
  findmaximaluniquematches of Vmengine/vmengineexport.h:4-81 call these.

  Conventions (the reference's, include/errordef.h:45-82): functions return
  0 on success and a negative code on error; the message is then available
  from vsa_messagespace().  All calls on one vsa_index must come from one
  thread at a time, like the reference's engine.
*/
#ifndef VSTREE_AMD_H
#define VSTREE_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSA_SEPARATOR 255u /* include/chardef.h:19 */
#define VSA_WILDCARD  254u /* include/chardef.h:25 */
#define VSA_UNDEFBWT  253u /* include/chardef.h:31,50 */
#define VSA_NO_SUBST  0xFFFFFFFFu

/* ---- errors: messagespace(), include/errordef.h:13 -------------------- */

const char *vsa_messagespace(void);

/* ---- the index: Virtualtree, include/virtualdef.h:186-219 ------------- */

/*
  Raw tables of one index exactly as mkvtree -allout writes them and
  mapvirtualtreeifyoucan (kurtz-basic/readvirt.c:776-907) maps them: host
  pointers, host endianness, no headers.  integersize is the bit width of
  the entries of suf, bck and llv (32 or 64, the `integersize=` line of the
  .prj file, Mkvtree/mkvprocess.c:403-504).  bwt may be NULL unless
  vsa_findmaximaluniquematches is used.
*/
typedef struct
{
  uint64_t totallength;     /* multiseq.totallength                     */
  uint32_t prefixlength;    /* Virtualtree.prefixlength                 */
  uint32_t numofchars;      /* alpha.mapsize - 1 (4 for DNA)            */
  uint32_t integersize;     /* 32 or 64                                 */
  uint64_t largelcpvalues;  /* pairs in llv                             */
  const uint8_t *tis;       /* [totallength]   alphabet-mapped text     */
  const void *suf;          /* [totallength+1] suffix array             */
  const uint8_t *lcp;       /* [totallength+1] min(lcp, 255)            */
  const void *llv;          /* [2*largelcpvalues] (index, value) pairs  */
  const void *bck;          /* [2*numofchars^prefixlength] (left, mid)  */
  const uint8_t *bwt;       /* [totallength+1] or NULL                  */
  /* indexes built with mkvtree -db G -q Q: position of the separator
     between database and queries (getqueryseppos,
     kurtz-basic/multiseq-adv.c:1005); ignored if hasindexedqueries == 0 */
  uint64_t querysepposition;
  int hasindexedqueries;
} vsa_tables;

typedef struct vsa_index vsa_index; /* ESA resident in one GPU's HBM */

/* uploads the tables to HIP device `device`; the host tables are not
   referenced after return */
int vsa_index_from_tables(const vsa_tables *tables, int device,
                          vsa_index **index);

/* reads indexname.prj and maps indexname.{tis,suf,lcp,llv,bck,bwt} like
   mapvirtualtreeifyoucan(…, TISTAB|SUFTAB|LCPTAB|BCKTAB[|BWTTAB])
   (kurtz-basic/readvirt.c:776, demand: Vmatch/mapdemand.c:174-191) */
int vsa_index_open(const char *indexname, int device, vsa_index **index);

void vsa_index_close(vsa_index *index);

/* A replica of an index on another HIP device of the node (or on the same
   one): every table, the derived search tables included, is copied device to
   device -- over xGMI between two GPUs -- and nothing is built again.  The
   multi-GPU entry points (include/vstree_amd_multi.h) replicate with it. */
int vsa_index_clone(const vsa_index *index, int device, vsa_index **clone);

typedef struct
{
  uint64_t totallength, numofcodes, largelcpvalues, device_bytes;
  uint32_t prefixlength, numofchars, device_integersize;
  int device, hasindexedqueries, hasbwt;
  /* symbols of the derived deep bucket table (esa8/slot16), 0 if
     this index has none and is searched probe for probe like the reference */
  uint32_t deepprefix;
} vsa_index_info;

int vsa_index_getinfo(const vsa_index *index, vsa_index_info *info);

/*
  Builds the tables on the GPU from an alphabet-mapped text that is already
  on the host (symbols 0..numofchars-1, VSA_WILDCARD, VSA_SEPARATOR), with
  the semantics of mkvtree -pl <prefixlength> -tis -suf -lcp -bck -bwt
  (Mkvtree/mkvprocess.c:875-1089; suffix order Mkvtree/bese.c:27-49,602).
  prefixlength 0 selects vm_recommendedprefixlength (kurtz/detpfxlen.c:52).
*/
int vsa_index_build(const uint8_t *tis, uint64_t totallength,
                    uint32_t numofchars, uint32_t prefixlength, int device,
                    vsa_index **index);

/*
  mkvtree on the GPU: reads multiple-FASTA files like
  `mkvtree -db dbfiles.. [-q queryfiles..] -indexname NAME -dna -pl [n] -allout`
  (Mkvtree/mkvtree.c:689, input Mkvtree/mkvinput.c:173, DNA symbol map) and
  writes NAME.{prj,al1,tis,ois,des,sds,ssp,suf,lcp,llv,bck,bwt,sti1[,skp]} byte
  for byte as the reference does (Mkvtree/mkvprocess.c:99-816); the reference's
  vmatch reads them.  prefixlength 0 = the reference's recommendation;
  integersize 64 matches the reference's LP64 build, 32 halves suf/bck/llv.
  Plain (uncompressed) FASTA only.
*/
int vsa_mkvtree(const char *const *dbfiles, uint32_t numofdbfiles,
                const char *const *queryfiles, uint32_t numofqueryfiles,
                const char *indexname, uint32_t prefixlength,
                uint32_t integersize, int withskp, int device);

/* same, for a text that already lives in device memory (bench.py) */
int vsa_index_build_device(const void *device_tis, uint64_t totallength,
                           uint32_t numofchars, uint32_t prefixlength,
                           int device, vsa_index **index);

/* table sti1 of mkvtree (Mkvtree/mkvprocess.c:583-612), computed on the GPU
   from suf and lcp into host memory sti1[totallength+1]; the GPU search does
   not use it, the reference's default algorithm (kurtz/matchsub.c:353) does */
int vsa_index_make_sti1(const vsa_index *index, uint8_t *sti1);

/* declares the text of a built index as "database, separator at
   querysepposition, queries" -- what mkvtree -db G -q Q records in the .prj
   file -- so that vsa_findmaximaluniquematches can run on it */
int vsa_index_set_queryseparator(vsa_index *index, uint64_t querysepposition);

/* Matchparam.queryspeedup (Vmengine/mparms.h:53, `vmatch -qspeedup`): which
   of the reference's algorithms the MEM lists (`-l L -q`) follow in their
   order inside one query offset -- 0 = matchquerysubstring0
   (kurtz/matchsub.c:165), 2 = matchquerysubstring2 (:353), the reference's
   default and the default here.  The set of matches is the same; complete
   matches, MUMs and MUM candidates do not depend on it.  Other values are an
   error ("illegal speedup value", Vmengine/fquery.c:433). */
int vsa_index_set_queryspeedup(vsa_index *index, uint32_t queryspeedup);

/* copies the device tables back to host buffers sized by the caller from
   vsa_index_getinfo (entries of suf/bck/llv have device_integersize bits);
   NULL pointers are skipped */
int vsa_index_download(const vsa_index *index, uint8_t *tis, void *suf,
                       uint8_t *lcp, void *llv, void *bck, uint8_t *bwt);

/* ---- queries: Queryinfo.multiseq, Vmengine/mparms.h:73-84 ------------- */

typedef struct vsa_queries vsa_queries;

/*
  nq query sequences given as (start, length) pairs into one buffer of
  alphabet-mapped symbols -- the layout of a reference Multiseq: sequences
  separated by VSA_SEPARATOR, start[i] = markpos[i-1]+1
  (include/multidef.h:113-133, kurtz-basic/multiseq.c:129-166).
  Contract: symbols are codes of the index's alphabet or >= 254 (wildcard,
  separator).  A batch is not bound to an index, so nothing checks this; a
  code in [numofchars, 253] would give a q-gram code beyond the bucket table.
*/
int vsa_queries_from_host(const uint8_t *symbols, uint64_t nsymbols,
                          const uint64_t *start, const uint64_t *length,
                          uint64_t nq, int device, vsa_queries **queries);

/* nq queries of equal length m stored back to back in device memory
   (device_symbols[i*m .. i*m+m)); the buffer is copied */
int vsa_queries_from_device(const void *device_symbols, uint64_t nq,
                            uint32_t m, int device, vsa_queries **queries);

/*
  Reads at two bits per symbol: what crosses PCIe and lies in HBM for a batch
  of short reads of ONE length m is a quarter of the Multiseq's bytes.
    row of read i = words [i * W, (i + 1) * W) of `rows`, W =
      vsa_packed_words(m) = ceil((2 m + 8) / 64) 64-bit words; symbol j in
      bits 63 - 2 (j mod 32), 62 - 2 (j mod 32) of word j / 32 -- the first
      symbol in the top bits, codes a 0, c 1, g 2, t 3 as the DNA symbol map
      assigns them (kurtz-basic/alphabet.c:369, `mkvtree -dna`); every other
      bit 0, except the lowest byte of the last word, the row's flag:
        0  all m symbols are bases
        1  the read holds a special symbol (a wildcard, kurtz/maxpref.c:30-41:
           it matches nothing, not even itself): the row's symbol bits are
           ignored, word 0 = k << 8 (the flag byte stays free where W = 1)
           names entry k of `special`, the read's m mapped symbols as bytes
           at special + k * m.
  vsa_pack_reads makes rows (and the side list) from numofqueries reads of m
  mapped symbols, read i at symbols + i * stride (stride = m: back to back;
  m + 1: a Multiseq with its separators); *numofspecial counts the entries of
  `special` in use, before and after (several calls -- several threads over
  disjoint pieces with side lists of their own, or one reader in turn -- fill
  one batch); -2 if specialcapacity does not suffice.  Host code, no GPU:
  eight symbols per step on CPUs with BMI2 (PEXT), about 60 M reads of 100
  symbols per second and thread.  vsa_pack_reads_mt does the same on `threads`
  host threads over disjoint pieces of the batch (the side list is numbered
  afterwards, in the order of the reads: the rows do not depend on the number
  of threads).
  A packed batch is a batch like any other to every engine call.  -complete,
  -mum and -mum cand on an index with deep tables read the rows directly
  (reads of up to 252 symbols: whole in registers up to 124, through 16-byte
  windows of the row beyond); the other modes and longer reads make the bytes
  on the device first (once per batch: 0.3 ms per 10 M reads of 100 symbols).
*/
uint32_t vsa_packed_words(uint32_t querylength);
int vsa_pack_reads(const uint8_t *symbols, uint64_t numofqueries,
                   uint32_t querylength, uint64_t stride, uint64_t *rows,
                   uint8_t *special, uint64_t specialcapacity,
                   uint64_t *numofspecial);
int vsa_pack_reads_mt(const uint8_t *symbols, uint64_t numofqueries,
                      uint32_t querylength, uint64_t stride, uint64_t *rows,
                      uint8_t *special, uint64_t specialcapacity,
                      uint64_t *numofspecial, uint32_t threads);
int vsa_queries_from_host_packed(const uint64_t *rows, uint64_t numofqueries,
                                 uint32_t querylength, const uint8_t *special,
                                 uint64_t numofspecial, int device,
                                 vsa_queries **queries);

/* vmatch -p: the batch with every sequence replaced by its reverse
   complement (symbol 3 - c, wildcards stay), what copymultiseqRC
   (kurtz-basic/readmulti.c:93-125) stores in Multiseq.rcsequence and the
   engine receives with rcmode = True (Vmatch/runquery.c:179-279).  A symbol
   above 3 that is not a wildcard is the reference's error "reverse
   complement of %lu undefined" (readmulti.c:45-49).  Match positions inside
   the query refer to the reverse complement; the flip back to the forward
   strand is the sink's (Vmatch/procfinal.c:152-168). */
int vsa_queries_reverse_complement(const vsa_queries *queries,
                                   vsa_queries **rcqueries);

void vsa_queries_free(vsa_queries *queries);

/* queryseq of every match = index in the batch + offset: a rank that holds
   queries [offset, offset+nq) of a larger job reports global numbers
   (the reference's onlinequerynumoffset, Vmengine/fquery.c:1010,
   Vmengine/initmstate.c:7-45) */
int vsa_queries_set_offset(vsa_queries *queries, uint64_t offset);

typedef struct
{
  uint64_t numofqueries, numofsymbols;
  uint64_t minlength, maxlength; /* of a query; 0, 0 for an empty batch      */
  uint64_t offset;               /* vsa_queries_set_offset                   */
  int device;
} vsa_queries_info;

int vsa_queries_getinfo(const vsa_queries *queries, vsa_queries_info *info);

/* ---- matches ---------------------------------------------------------- */

/* field for field the reference's MUMcandidate (include/mumcand.h:17-23);
   what processexactquerymatch(info, l, i, queryseq, querystart)
   (Vmengine/procexqu.c:17-64) receives for one match */
typedef struct
{
  uint64_t length;     /* length1 = length2                           */
  uint64_t dbstart;    /* position1: absolute position in the index   */
  uint64_t queryseq;   /* seqnum2                                     */
  uint64_t querystart; /* relpos2                                     */
} vsa_match;

typedef struct vsa_result vsa_result; /* match list resident in HBM */

typedef struct
{
  uint64_t count;          /* matches                                     */
  uint64_t sumlength;      /* sum of match lengths ("bp matched")         */
  uint64_t searches;       /* bucket lookups + binary searches performed  */
  uint64_t candidates;     /* MUM candidates before the query-side filter */
  double search_kernel_ms; /* HIP-event time of the dominant search kernel */
  double total_device_ms;  /* HIP-event time of the whole call            */
  double anchor_ms;        /* -mum: anchor pass + work list (0 if unused)  */
  uint64_t kernel_searches; /* of those: by the dominant search kernel     */
  double first_kernel_ms;  /* -mum: HIP-event time of the first pass kernel
                              (offset 0 of every query, whole query);
                              -complete -e/-h: of the banded alignment     */
} vsa_stats;

uint64_t vsa_result_count(const vsa_result *result);
int vsa_result_getstats(const vsa_result *result, vsa_stats *stats);
/* copies min(count, capacity) matches to the host, in reference order */
int vsa_result_fetch(const vsa_result *result, vsa_match *matches,
                     uint64_t capacity);
const void *vsa_result_device_matches(const vsa_result *result);
/* device-to-device copy of min(count, capacity) matches into caller memory
   (e.g. a torch tensor that then goes through an RCCL collective) */
int vsa_result_copy_device(const vsa_result *result, void *device_matches,
                           uint64_t capacity);
void vsa_result_free(vsa_result *result);
/* a match list from host memory (fetched earlier, filtered or made by the
   caller) as a result on HIP device `device`: for the consumers of results
   that stay on the device (vsa_coverage_mark) */
int vsa_result_from_host(const vsa_match *matches, uint64_t count, int device,
                         vsa_result **result);

/* ---- the engine: Vmengine/vmengineexport.h:4-81 ----------------------- */

/*
  findcompletematches (Vmengine/fcomplete.c:263-321) for exact matching on
  the index (decidefcm -> findexactcompletematchesindex,
  Vmengine/exactcompl.c:168-239).  Order: query order, within a query suffix
  array order.  A query shorter than prefixlength is the reference's hard
  error "patternlength=%lu must be >= %lu=prefixlen" (exactcompl.c:179-185):
  the matches of the queries before it are delivered, the return code is
  negative.  In every match length = query length and querystart = 0.
*/
int vsa_findcompletematches(const vsa_index *index,
                            const vsa_queries *queries, vsa_result **result);

/*
  The MUM candidates of a batch (vmatch -mum cand -l L), in reference order or
  -- ordered = 0 -- as the search kernel left them, for callers that hand
  them to a filter which sorts them anyway: the multi-GPU form of vmatch -mum
  (kurtz/cleanMUMcand.c:55-118 range-partitioned over the ranks, DESIGN.md
  section 6).
*/
int vsa_findmumcandidates(const vsa_index *index, const vsa_queries *queries,
                          uint64_t searchlength, int ordered,
                          vsa_result **result);

/*
  The same candidates as PAIRS of 8-byte words, never as 32-byte records:
    key   = dbstart << lengthbits | (2^lengthbits - 1 - length)
    value = queryseq << 16 | querystart
  -- what the filter sorts by, and what it needs to write a record once a
  candidate has survived.  lengthbits: the same on every rank of a job, at
  least the bits of the longest query anywhere (at most 16); 0 = the bits of
  this batch's longest query.  The result is for vsa_result_partition, which
  then writes rows of the two words (half the bytes of the exchange);
  vsa_result_fetch / vsa_result_copy_device deliver it as records,
  vsa_result_device_matches is NULL for it.
  Limits of the pair form: queries shorter than 65 535 symbols and global
  query numbers below 2^48; a batch beyond them is answered with -2 and a
  message, and the caller takes the record form -- vsa_findmumcandidates,
  vsa_result_partition on records, vsa_mumuniqueinquery_range -- as
  vsa_multi_findmatches (multi_gpu.cpp) does by itself.
*/
int vsa_findmumcandidates_packed(const vsa_index *index,
                                 const vsa_queries *queries,
                                 uint64_t searchlength, uint32_t lengthbits,
                                 vsa_result **result);
/* the lengthbits of a packed result, 0 for a result of records */
uint32_t vsa_result_packbits(const vsa_result *result);

/*
  The records of a result grouped by the range of the index their dbstart
  falls into -- part p = floor(dbstart * nparts / (totallength + 1)), equal
  dbstarts in the same part -- written to device_matches (room for
  vsa_result_count records) part by part; counts[p] (host, nparts entries) =
  records of part p; maxright[p] (host, may be NULL) = the largest right end
  dbstart + length - 1 among them, 0 if there is none.  The send buffer and
  the split sizes of the all-to-all that brings every candidate to the rank
  filtering its range, and what the ranks need to agree on the carry of
  vsa_mumuniqueinquery_range without looking at the records again.
*/
int vsa_result_partition(const vsa_result *result, uint32_t nparts,
                         uint64_t totallength, void *device_matches,
                         uint64_t *counts, uint64_t *maxright);
/* ... with the part `ownpart` (0 .. nparts-1) written behind all others, the
   others in ascending order in front of it: a rank's own candidates stay
   where they are, the rows in front of them are the send buffer of an
   all-to-all whose split for the rank itself is 0.  counts and maxright are
   indexed by part as above.  ownpart < 0: vsa_result_partition. */
int vsa_result_partition_own(const vsa_result *result, uint32_t nparts,
                             int ownpart, uint64_t totallength,
                             void *device_matches, uint64_t *counts,
                             uint64_t *maxright);
/* ... with the 2 * nparts numbers -- counts[0 .. nparts-1], then
   maxright[0 .. nparts-1] -- left in DEVICE memory (device_meta), where the
   all-gather of the ranks reads them: the call does not wait for the GPU.
   STREAM CONTRACT: the work is queued on the device's default (NULL) stream
   and nothing else orders it: whoever reads device_matches / device_meta does
   so on that stream (a copy or collective queued there), or synchronises
   with it first (hipStreamSynchronize(NULL) / an event recorded there).  A
   non-blocking stream of the caller's is NOT ordered behind it.  The same
   holds for the rows vsa_mumuniqueinquery_range_packed[2] reads: they must
   be complete on the default stream's terms when the call is made. */
int vsa_result_partition_device(const vsa_result *result, uint32_t nparts,
                                int ownpart, uint64_t totallength,
                                void *device_matches, uint64_t *device_meta);
/* vsa_findmumcandidates_packed and vsa_result_partition_device (totallength
   = that of the index) in one call, for a caller that keeps its row buffer
   from batch to batch: 0 = the rows (vsa_result_count(*result) of them) lie
   grouped in device_rows; 1 = there are more than `capacity` rows: nothing
   was grouped, *result holds the candidates (make room, then
   vsa_result_partition_device); < 0 as vsa_findmumcandidates_packed. */
int vsa_findmumcandidates_grouped(const vsa_index *index,
                                  const vsa_queries *queries,
                                  uint64_t searchlength, uint32_t lengthbits,
                                  uint32_t nparts, int ownpart,
                                  void *device_rows, uint64_t capacity,
                                  uint64_t *device_meta, vsa_result **result);

/*
  findcompletematches for approximate matching on the index, vmatch
  -complete -e K | -h K -q Q IDX: decidefcm -> findedistcompletematchesindex
  / findhammingcompletematchesindex (Vmengine/fcomplete.c:140-261) ->
  findapproxcompletematchesindex (Vmengine/approxcompl.c:138-199) ->
  splitesaapm (Vmengine/splitesaapm.c:458-558).
    doedist   1: edit distance (-e), 0: Hamming distance (-h)
    distvalue K;  percent 1: the threshold is m*K/100 (-e Kp, -h Kp,
              Vmengine/initcompl.c:52-56); percent 2: "best of" (-e Kb, -h Kb,
              initcompl.c:59-77) -- read by read (Vmengine/fcomplete.c:251-252
              restores K in front of every read) the smallest threshold
              t <= m*K/100 at which the read has a match at all
              (Vmengine/approxcompl.c:80-122), then the read's matches at
              threshold t; a read without one reports nothing.  Two passes
              here: the smallest distance of every read from a run at the
              percent thresholds, then every read at exactly its own
  A match is (length, dbstart, queryseq, distance): length = Match.length1
  (for -e the best-distance, then longest prefix behind dbstart,
  Vmengine/longestmatch.c; for -h the query length), the distance travels in
  the querystart field (the number of mismatches for -h, where the reference
  stores its negative in Match.distance, approxcompl.c:78).  Order: query
  order; within a query the merged candidate regions in ascending order,
  within a region DESCENDING dbstart, exactly as the reference's right-to-left
  verification reports them.
  Errors: a threshold >= query length is the reference's
  "threshold=%lu>=%lu=patternlen not allowed" (splitesaapm.c:496-501): the
  matches of the queries before it are delivered, the return code is -2.
  Patterns that are not cut (splitsize 1: short patterns -- reported in
  suffix array order, splitesaapm.c:523-543) and pieces with a threshold of
  their own (K >= m/10), i.e. what the reference hands to esaapm /
  esahamming, and Hamming distance with a wildcard in a read take a general
  path (a depth-first walk of the lcp-interval tree per piece,
  approx_tree.inc) instead of the pigeonhole path; a batch with ONE such
  query takes it as a whole.
  Reads whose threshold is 0 (-e Kp / -h Kp on short reads) are exact
  searches (approxcompl.c:167-176), also inside a batch whose other reads
  have thresholds > 0: the batch is cut into the two kinds and the lists are
  merged back into query order; the first read the reference would stop at
  (shorter than prefixlength with threshold 0, or threshold >= length) ends
  the run with its message, -2, and the matches of the reads before it.
  Text positions are kept in the width of the index tables: texts of 2^32
  symbols and more are searched like the others.
  VSA_NOT_COVERED (-4), no result: the configuration is one this engine does
  not implement (alphabets other than 4 symbols; a read of more than 512
  symbols; a batch of 2^31 reads and more, or more reads than
  bits(reads) + bits(text length) <= 64 allows) -- the caller keeps using its
  CPU function for such batches (integration/vmengine_shim.c does).
*/
#define VSA_NOT_COVERED (-4)
int vsa_findapproxcompletematches(const vsa_index *index,
                                  const vsa_queries *queries, int doedist,
                                  uint64_t distvalue, int percent,
                                  vsa_result **result);

/*
  findquerymatches (Vmengine/fquery.c:1009-1058) for exact matches:
    domaximaluniquematch = 0                      vmatch -l L        (MEM)
    domaximaluniquematch = 1, ...candidates = 1   vmatch -mum cand -l L
    domaximaluniquematch = 1, ...candidates = 0   vmatch -mum -l L
  searchlength is Matchparam.seedlength (Vmatch/matchlenparm.c:17-22); a
  value below prefixlength is the reference's error (fquery.c:440-446).
  Order: MEM and candidates by query, query offset, then witness / left /
  right like kurtz/matchsub.c with Vmengine/fquery.c:139-270 (the witness is
  that of the reference's default algorithm 2, or of algorithm 0 after
  vsa_index_set_queryspeedup(index, 0)); MUMs by ascending dbstart
  (kurtz/cleanMUMcand.c:55-118).
*/
int vsa_findquerymatches(const vsa_index *index, const vsa_queries *queries,
                         int domaximaluniquematch,
                         int domaximaluniquematchcandidates,
                         uint64_t searchlength, vsa_result **result);

/*
  findselfmatches with vmatmaxoutgeneric (Vmengine/fself.c:203-300,
  Vmengine/vmatfind.c:487-541), vmatch -l L IDX: maximal repeats of the
  index -- all pairs of positions whose common prefix has length >= L, cannot
  be extended to the right (its length is the reported one) and is left
  maximal (different left characters, or a special symbol / the start of the
  text on one side).  A match is (length, start1, start2, 0) with start1 <
  start2.  Order: the reference's -- attachments of children to their fathers
  in the order of its bottom-up traversal, the pairs of one attachment in the
  order of the nested loops of processbranch (vmatfind.c:433-469).  With
  queries inside the index only pairs of a database and a query position are
  reported (ACCEPTMATCH, fself.c:29-37).  Needs the bwt table.
  VSA_NOT_COVERED for alphabets of more than 32 symbols.
*/
int vsa_findmaximalrepeats(const vsa_index *index, uint64_t searchlength,
                           vsa_result **result);

/*
  findsupermax (Vmengine/fsuper.c:142-165), vmatch -supermax -l L IDX:
  supermaximal repeats of the index.  A match is (length, start1, start2, 0)
  with start1 < start2, laid out like the self-index MUMs (dbstart = start1,
  queryseq = start2 as an absolute position).  Order: the nodes of the
  lcp-interval tree in suffix array order, the pairs of a node by first,
  then second suffix -- the reference's order.  An index that holds queries
  is the reference's error "supermaximal repeat search does not allow query
  files in index" (Vmengine/fself.c:193-198).  Needs the bwt table.
*/
int vsa_findsupermaximalrepeats(const vsa_index *index, uint64_t searchlength,
                                vsa_result **result);

/*
  findtandems (Vmengine/ftandem.c:261-304), vmatch -tandem -l L IDX: right
  branching tandem repeats -- every position v where a string of length
  d >= L that names an lcp-interval occurs twice in a row and the repeat
  cannot be shifted right by one symbol.  A match is (d, v, v + d, 0), laid
  out like the other self matches.  Order: the lcp-intervals as the
  reference's bottom-up traversal completes them, the repeats of one interval
  from the reference's witness leftwards, then rightwards.  An index that
  holds queries is the reference's error "tandem repeat search does not allow
  query files in index" (ftandem.c:271-275).  Needs tis, suf, lcp (llv).
*/
int vsa_findtandems(const vsa_index *index, uint64_t searchlength,
                    vsa_result **result);

/*
  findmaximaluniquematches (Vmengine/fmumself.c:10-66): MUMs between the
  database and the query part of one index.  Reported like the reference's
  Outputfunction(outinfo, len, start1, start2): length, dbstart = start1,
  queryseq = start2 (absolute), querystart = 0; suffix array order.
  VSA_NOT_COVERED for alphabets of more than 128 symbols (mkvtree -smap with
  such a map: the reference's engine keeps those).
*/
int vsa_findmaximaluniquematches(const vsa_index *index,
                                 uint64_t searchlength, vsa_result **result);

/*
  The same scan over a part of the suffix array: the values first <= i < last
  of the reference's loop variable (fmumself.c:33 runs i = 2 .. totallength-1;
  the bounds are clamped to that).  This is the multi-GPU form:
  every rank holds the whole index, rank r of N scans
  [2 + r*(n-2)/N, 2 + (r+1)*(n-2)/N) -- the entries i-2, i-1, i around the ends
  of its range ("halo") come from its own copy of lcptab/bwttab -- and the
  lists of the ranks, concatenated in rank order, are the list of the whole
  scan; only the match counters are reduced.
*/
int vsa_findmaximaluniquematches_range(const vsa_index *index,
                                       uint64_t searchlength, uint64_t first,
                                       uint64_t last, vsa_result **result);

/*
  mumuniqueinquery (kurtz/cleanMUMcand.c:55-118) on its own: MUM candidates
  resident in device memory (any order; e.g. gathered from several GPUs) ->
  MUMs in ascending dbstart order.  The candidate buffer is reordered.
*/
int vsa_mumuniqueinquery(void *device_candidates, uint64_t ncandidates,
                         int device, vsa_result **result);

/*
  The same filter on ONE dbstart range of a job whose candidates are
  partitioned by dbstart over several GPUs: carry_dbright = the largest
  right end (dbstart + length - 1) among all candidates with a smaller
  dbstart, i.e. the value the reference's running variable `dbright`
  (kurtz/cleanMUMcand.c:63,90) has when its loop reaches this range.  Equal
  dbstarts must not be split between ranges.
*/
int vsa_mumuniqueinquery_range(void *device_candidates, uint64_t ncandidates,
                               int device, uint64_t carry_dbright,
                               vsa_result **result);
/* ... on rows of (key, value) pairs as vsa_result_partition wrote them for a
   packed result; totallength = that of the index.  The MUMs are records. */
int vsa_mumuniqueinquery_range_packed(const void *device_rows, uint64_t nrows,
                                      uint32_t lengthbits,
                                      uint64_t totallength, int device,
                                      uint64_t carry_dbright,
                                      vsa_result **result);
/* ... on two lists of such rows taken as one (a rank's own rows, which need
   not travel through the exchange, and the rows it received) */
int vsa_mumuniqueinquery_range_packed2(const void *device_rows, uint64_t nrows,
                                       const void *more_rows, uint64_t nmore,
                                       uint32_t lengthbits,
                                       uint64_t totallength, int device,
                                       uint64_t carry_dbright,
                                       vsa_result **result);

/*
  The same three entry points with the reference's delivery model: every
  match is handed to a callback on the calling thread, in reference order;
  a non-zero return stops the run and is propagated
  (Processfinalfunction, include/match.h:232; procexqu.c:61).
*/
typedef int (*vsa_processmatch)(void *info, const vsa_match *match);

int vsa_findcompletematches_cb(const vsa_index *index,
                               const vsa_queries *queries,
                               vsa_processmatch processmatch, void *info);
int vsa_findapproxcompletematches_cb(const vsa_index *index,
                                     const vsa_queries *queries, int doedist,
                                     uint64_t distvalue, int percent,
                                     vsa_processmatch processmatch,
                                     void *info);
int vsa_findquerymatches_cb(const vsa_index *index,
                            const vsa_queries *queries,
                            int domaximaluniquematch,
                            int domaximaluniquematchcandidates,
                            uint64_t searchlength,
                            vsa_processmatch processmatch, void *info);
int vsa_findmaximaluniquematches_cb(const vsa_index *index,
                                    uint64_t searchlength,
                                    vsa_processmatch processmatch,
                                    void *info);
int vsa_findsupermaximalrepeats_cb(const vsa_index *index,
                                   uint64_t searchlength,
                                   vsa_processmatch processmatch, void *info);
int vsa_findmaximalrepeats_cb(const vsa_index *index, uint64_t searchlength,
                              vsa_processmatch processmatch, void *info);
int vsa_findtandems_cb(const vsa_index *index, uint64_t searchlength,
                       vsa_processmatch processmatch, void *info);

/* ---- end to end: queries in host memory -> matches in host memory ------
   Three batches in flight: while one is searched, the next is uploaded and
   the matches of the one before are downloaded (page-locked buffers the caller
   fills and reads in place, one HIP stream per direction).  Reads of one
   length, packed back to back.  mode: 0 -complete, 1 -l L (MEM), 2 -mum cand,
   3 -mum (candidates of all batches stay on the device; the filter of
   kurtz/cleanMUMcand.c:55-118 runs once, in vsa_pipeline_finish).  queryseq
   of a match counts over all batches (Vmengine/fquery.c:1010
   onlinequerynumoffset).
   Jobs: vsa_pipeline_finish and vsa_pipeline_finish16 end a -mum job, also
   when they report that a batch of it failed: the candidates are dropped and
   the reads of the next job are numbered from 0 again.  Modes 0 to 2 have no
   job end; their numbering goes on until vsa_pipeline_set_offset(p, 0).
   VSA_PIPELINE_ROW_SLACK in the environment of vsa_pipeline_open (tests): the
   device buffer of the -mum candidates grows to the rows it must hold and
   that many more, instead of twice the rows and 2^20 more.

     vsa_pipeline_open(index, 3, 20, 100, 10000000, &p);
     while (more reads) {
       uint8_t *buf;
       while ((buf = vsa_pipeline_hostbuffer(p)) == NULL)
         vsa_pipeline_next(p, &m, &n);          -- take a finished batch
       n_reads = fill(buf);  vsa_pipeline_submit(p, n_reads);
     }
     while (vsa_pipeline_next(p, &m, &n) != 1) ...;
     vsa_pipeline_finish(p, &mums, &nmums, &stats);                        */
typedef struct vsa_pipeline vsa_pipeline;
int vsa_pipeline_open(const vsa_index *index, int mode, uint64_t searchlength,
                      uint32_t querylength, uint64_t maxqueries,
                      vsa_pipeline **pipeline);
uint8_t *vsa_pipeline_hostbuffer(vsa_pipeline *pipeline);
int vsa_pipeline_submit(vsa_pipeline *pipeline, uint64_t numofqueries);
/* The same pipeline for reads at two bits per symbol (vsa_pack_reads): a
   quarter of the bytes cross PCIe and lie in HBM.  The caller packs into the
   slot's page-locked room -- *rows: maxqueries rows of vsa_packed_words(m)
   words, *special: maxspecial reads as bytes -- and submits the numbers it
   used.  vsa_pipeline_hostrows: 0 = a slot, 1 = all three batches are in
   flight (take results first).  Everything else as above. */
int vsa_pipeline_open_packed(const vsa_index *index, int mode,
                             uint64_t searchlength, uint32_t querylength,
                             uint64_t maxqueries, uint64_t maxspecial,
                             vsa_pipeline **pipeline);
int vsa_pipeline_hostrows(vsa_pipeline *pipeline, uint64_t **rows,
                          uint8_t **special);
int vsa_pipeline_submit_packed(vsa_pipeline *pipeline, uint64_t numofqueries,
                               uint64_t numofspecial);
/* 0: the oldest batch not yet delivered (host memory, valid until the next
   call that needs its slot); 1: nothing outstanding; < 0: that batch failed
   (message in vsa_messagespace(), matches up to the error delivered) */
int vsa_pipeline_next(vsa_pipeline *pipeline, const vsa_match **matches,
                      uint64_t *count);
int vsa_pipeline_finish(vsa_pipeline *pipeline, const vsa_match **matches,
                        uint64_t *count, vsa_stats *stats);
/* the same list at 16 bytes per MUM -- half the bytes on the host link, which
   is what a -mum job of short reads waits for at its end: reads of up to
   65 535 symbols, texts below 2^40 symbols */
typedef struct
{
  uint64_t dbstart_length;      /* dbstart << 24 | length */
  uint64_t queryseq_querystart; /* queryseq << 16 | querystart */
} vsa_match16;
#define VSA_MATCH16_LENGTH(x) ((x).dbstart_length & 0xFFFFFFull)
#define VSA_MATCH16_DBSTART(x) ((x).dbstart_length >> 24)
#define VSA_MATCH16_QUERYSEQ(x) ((x).queryseq_querystart >> 16)
#define VSA_MATCH16_QUERYSTART(x) ((x).queryseq_querystart & 0xFFFFull)
int vsa_pipeline_finish16(vsa_pipeline *pipeline, const vsa_match16 **matches,
                          uint64_t *count, vsa_stats *stats);
void vsa_pipeline_close(vsa_pipeline *pipeline);

/* For a caller that runs one pipeline per GPU and deals the batches of a job
   out to them (include/vstree_amd_multi.h, vsa_multi_pipeline_*):
   vsa_pipeline_set_offset: the number the first query of the NEXT submitted
   batch gets.  vsa_pipeline_take_candidates (-mum pipelines, all batches
   taken): the candidate rows of the job where they lie in device memory -- 16
   bytes each, sort key dbstart << lengthbits | (2^lengthbits - 1 - length) and
   value queryseq << 16 | querystart, valid until the next batch is submitted
   -- instead of vsa_pipeline_finish; ends the job, but leaves the numbering
   of the next one to the caller (vsa_pipeline_set_offset).
   vsa_rows_partition_device: such rows grouped by the range of the index
   their dbstart falls into, like vsa_result_partition_device (same stream
   contract: the device's default stream). */
int vsa_pipeline_set_offset(vsa_pipeline *pipeline, uint64_t firstquery);
int vsa_pipeline_take_candidates(vsa_pipeline *pipeline,
                                 const void **device_rows, uint64_t *nrows,
                                 uint32_t *lengthbits);
int vsa_rows_partition_device(const void *device_rows, uint64_t nrows,
                              uint32_t lengthbits, uint32_t nparts,
                              int ownpart, uint64_t totallength, int device,
                              void *device_out, uint64_t *device_meta);

/* ---- synthetic inputs (bench.py, tests): SURVEY.md section 8d ---------- */

uint64_t vsa_splitmix64_at(uint64_t seed, uint64_t idx);
void vsa_synth_genome(uint64_t seed, uint64_t n, uint8_t *codes);
void vsa_synth_query_plan(uint64_t seed, uint64_t n, uint64_t nq, uint32_t m,
                          uint64_t *pos, uint32_t *substidx, uint8_t *step);
void vsa_synth_queries(uint64_t seed, const uint8_t *genome, uint64_t n,
                       uint64_t nq, uint32_t m, uint8_t *queries,
                       uint64_t *srcpos);
/* device-side generators writing into caller-provided device memory */
int vsa_synth_genome_device(uint64_t seed, uint64_t n, void *device_codes,
                            int device);
int vsa_synth_queries_device(const void *device_genome, uint64_t n,
                             const uint64_t *pos, const uint32_t *substidx,
                             const uint8_t *step, uint64_t nq, uint32_t m,
                             void *device_queries, int device);

/* plain device memory for callers without a HIP runtime of their own */
int vsa_device_malloc(uint64_t bytes, int device, void **ptr);
int vsa_device_free(void *ptr, int device);
int vsa_device_upload(void *device_dst, const void *host_src, uint64_t bytes,
                      int device);
int vsa_device_download(void *host_dst, const void *device_src, uint64_t bytes,
                        int device);
int vsa_device_count(void);
int vsa_device_synchronize(int device);
/* temporaries and freed result lists are recycled inside the library; this
   hands the cached device memory back to HIP */
int vsa_device_trim(int device);
/* what HIP reports as free / total memory of the device (the library's own
   cache of freed blocks counts as used until vsa_device_trim): how much room
   an index has, and what a failed job must leave unchanged */
int vsa_device_meminfo(int device, uint64_t *freebytes, uint64_t *totalbytes);
/* measured device-to-device streaming read rate in GB/s (roofline
   denominator cross-check in bench.py) */
int vsa_measure_stream_read(uint64_t bytes, int device, double *gbps);
/* independent random 8-byte reads over a table of `bytes` bytes, `inflight`
   (1, 4 or 8) of them issued per work-item before any is used: 10^9 reads
   per second.  The ceiling for the search kernels, whose traffic is one
   64-byte sector per read that misses the caches. */
int vsa_measure_random_read(uint64_t bytes, int inflight, int device,
                            double *greads);
/* the same reads over a table of a live index, where it lies in device
   memory: 0 slot16 (16-byte reads), 1 esa8, 2 tis2, 3 suf */
int vsa_measure_table_read(const vsa_index *ix, int table, int inflight,
                           double *greads);

/* ---- host match sink: from match records to vmatch's output lines ------ */

/*
  processfinal (Vmatch/procfinal.c:515-637: fetchpositions, convertthematch,
  assignEvalue, matchokay) and the default output line of
  vmatchnormaloutmatch (Vmatch/echomatch.c:878-987)
      len1 seq1 pos1 D|P len2 seq2 pos2 dist evalue score identity
  for the matches of this path, byte for byte what vmatch prints behind its
  "# args=" line (tests/test_sink.py: md5 of the lines of every golden run).
  Host side, no GPU involved; large batches are formatted by several
  threads, the text comes out in the order of the records.
  totalquerylength of an index with queries = totallength - (position of
  the separator in front of the first query sequence) - 1.
*/
#define VSA_SINK_COMPLETE       0 /* vsa_findcompletematches              */
#define VSA_SINK_QUERY          1 /* vsa_findquerymatches (-l, -mum ...)  */
#define VSA_SINK_SELF           2 /* vsa_findmaximaluniquematches         */
#define VSA_SINK_APPROX_EDIST   3 /* vsa_findapproxcompletematches, -e    */
#define VSA_SINK_APPROX_HAMMING 4 /* vsa_findapproxcompletematches, -h    */
/* vmatch -dnavsprot: records as the engine delivers them on a six-frame
   batch (vsa_queries_translate; queryseq counts the six frames of every DNA
   sequence, without an offset), the index a protein index.  numofqueries,
   querystart, querylength and querytotallength describe the DNA Multiseq,
   numofchars is the protein alphabet's.  Every record is converted
   (sixframeconvertmatch, Vmatch/procfinal.c:262-289) and printed with length2
   = 3 * length, the forward-strand position in the DNA sequence and the flag
   F (forward frame) or G (reverse frame) in place of D|P; E-value from the
   multiplier totallength * length of the DNA sequence and lenmatch = length2
   (procfinal.c:196-258), score = length1 + length2.  palindromic must be 0.
   vsa_select_*, vsa_cluster_*, vsa_matchcluster_* and vsa_chain_* answer
   VSA_NOT_COVERED for a layout of this kind.
   VSA_SINK_TRANSLATED_COMPLETE: the same for the records of
   vsa_findcompletematches on such a batch (-dnavsprot -complete), whose
   E-value has the multiplier totallength alone, as for VSA_SINK_COMPLETE. */
#define VSA_SINK_TRANSLATED     5
#define VSA_SINK_TRANSLATED_COMPLETE 6

/* Vmatch option -> bit of showmode (include/outinfo.h SHOW...) */
#define VSA_SHOW_ABSOLUTE   1u /* -absolute   */
#define VSA_SHOW_NODIST     2u /* -nodist     */
#define VSA_SHOW_NOEVALUE   4u /* -noevalue   */
#define VSA_SHOW_NOSCORE    8u /* -noscore    */
#define VSA_SHOW_NOIDENTITY 16u /* -noidentity */

typedef struct
{
  int kind;              /* VSA_SINK_...                                  */
  int palindromic;       /* matches of the reverse-complement pass (-p)   */
  int selfpalindromic;   /* ... of the index against itself (vmatch -p IDX,
                            Vmatch/runself.c:127-178): the query set is the
                            index; of the two mirror images of a match only
                            the one with the smaller left position is kept
                            (procfinal.c:159-167)                         */
  uint32_t showmode;     /* VSA_SHOW_... bits                             */
  uint32_t numofchars;   /* alpha.mapsize - 1: E-value match probability  */
  int threads;           /* formatting threads; 0 = one per processor     */
  uint64_t leastlength;  /* Matchparam.userdefinedleastlength (-l), or 0  */
  /* the index (Multiseq of the Virtualtree): */
  uint64_t totallength, numofsequences;
  const uint64_t *markpos;      /* numofsequences - 1 separator positions
                                   (IDX.ssp)                              */
  uint64_t numofquerysequences; /* sequences of queries INSIDE the index  */
  uint64_t totalquerylength;    /* their total length (IDX.prj), else 0   */
  /* the query set (not for VSA_SINK_SELF): sequence i occupies
     [querystart[i], querystart[i] + querylength[i]) of a Multiseq of
     querytotallength symbols */
  uint64_t numofqueries, querytotallength;
  const uint64_t *querystart, *querylength;
} vsa_sinkparams;

typedef struct vsa_sink vsa_sink;

int vsa_sink_open(const vsa_sinkparams *params, vsa_sink **sink);
void vsa_sink_close(vsa_sink *sink);
/* lines (each ending in a newline) into buffer; returns the bytes written or
   a negative code */
int64_t vsa_sink_format(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                        char *buffer, uint64_t capacity);
/* the same to a FILE * */
int vsa_sink_write(vsa_sink *sink, const vsa_match *matches, uint64_t n,
                   void *file);

/* ---- match coverage: vmatch -dbnomatch / -qnomatch / -dbmaskmatch /
   -qmaskmatch (Vmatch/markmat.c, nomatch.c, showmasked.c,
   initpost.c:28-74,156-267) on match lists that stay in HBM ---------------

   A vsa_coverage is the reference's marktable (Markinfo.markmatchtable,
   Vmatch/markinfo.h) in device memory, in a layout of our own: ONE BIT PER
   POSITION of a Multiseq, position p = bit (p & 63) of the 64-bit word
   p >> 6 (LSB first), the bits behind the last position 0.  Word index and
   bit arithmetic are 64 bit: tables of 2^32 bits and more are addressed like
   the others.  The positions of the separators are set from the start
   (initmarktable, markmat.c:15-28), so no run of clear bits spans two
   sequences. */

typedef struct vsa_coverage vsa_coverage;

/* initmarktable over the Multiseq of the index: totallength bits, the
   numofsequences - 1 separator positions set */
int vsa_coverage_open_index(const vsa_index *index, vsa_coverage **coverage);
/* ... over the query Multiseq as the reference lays it out
   (kurtz-basic/multiseq.c:129-166): sequence i starts at the sum of
   (length_j + 1) over j < i, whatever the batch looks like in memory (byte
   batches, uniform and dense batches, packed batches).  The offset of the
   batch (vsa_queries_set_offset) at the time of the call is subtracted from
   the queryseq of every match marked later. */
int vsa_coverage_open_queries(const vsa_queries *queries,
                              vsa_coverage **coverage);
void vsa_coverage_close(vsa_coverage *coverage);
uint64_t vsa_coverage_numofbits(const vsa_coverage *coverage);

#define VSA_COVERAGE_QUERY  0 /* dbstart absolute, queryseq / querystart
                                 relative, length for both instances:
                                 vsa_findquerymatches, vsa_findcompletematches */
#define VSA_COVERAGE_SELF   1 /* dbstart = start1, queryseq = start2, both
                                 absolute in the index: maximal, supermaximal
                                 and tandem repeats, self-index MUMs          */
#define VSA_COVERAGE_APPROX 2 /* vsa_findapproxcompletematches: database
                                 instance only, length = length1, the
                                 querystart field is a distance               */
#define VSA_COVERAGE_DATABASE 0 /* -dbnomatch / -dbmaskmatch: markdb = True  */
#define VSA_COVERAGE_QUERIES  1 /* -qnomatch / -qmaskmatch:   markdb = False */

/* an instance of at least this many positions is set by a whole wavefront,
   a shorter one by the lane that holds its record */
#define VSA_COVERAGE_COOP_THRESHOLD 1024u
uint64_t vsa_coverage_coop_threshold(void);
/* positions one workgroup of the extraction kernels looks at */
#define VSA_COVERAGE_EXTRACT_TILE 65536u

/*
  Markfields (Vmatch/markinfo.h:13-23) and what markmatches
  (Vmatch/markmat.c:42-118) reads besides: the four keep flags are 1 by
  default (DEFAULTMARKFIELDS, Vmatch/parsevm.c:83-87); `keepleft` clears
  markleft, `keepright` markright, `keepleftifsamesequence`
  markleftifdifferentsequence, `keeprightifsamesequence`
  markrightifdifferentsequence (Vmatch/keepflags.c:9-27).
    self layout   hasnoqueryfiles holds: both instances go into the table of
                  the index -- the left one if markleft and (markleftif... or
                  the two sequence numbers differ), the right one likewise.
                  On an index with queries Storeposition2 and Storeseqnum2
                  count from the first query sequence (procfinal.c:463-469);
                  the database side marks the right instance at that relative
                  position, as the reference does; the query side needs such
                  an index ("option -qnomatch requires index containing query
                  sequences or option -q", initpost.c:48-62) and marks the
                  right instance at its absolute position.
    query layout  (-q) the database side marks the left instance if markleft,
                  the query side the right instance in a table over the
                  queries, moved to seqlength - (querystart + length) if
                  palindromic (procfinal.c:152-158).  The two same-sequence
                  flags must be 1: with -q their keywords are the reference's
                  error (parsevm.c:70-80), which is returned (-2).
    approximate   the database side like the query layout.
  VSA_NOT_COVERED, table untouched: a packed-pair result; selfpalindromic
  lists; the query side of -complete lists (complete != 0 or the approximate
  layout: the reference marks query offsets in a table of the database there,
  initpost.c:25-26,66-70).
*/
typedef struct
{
  int layout;          /* VSA_COVERAGE_QUERY | _SELF | _APPROX             */
  int side;            /* VSA_COVERAGE_DATABASE | _QUERIES                  */
  int palindromic;     /* matches of the reverse-complement pass (-p)      */
  int selfpalindromic; /* vmatch -p IDX: not covered                       */
  int complete;        /* the list comes from vsa_findcompletematches      */
  int markleft, markright;
  int markleftifdifferentsequence, markrightifdifferentsequence;
} vsa_coverageparams;

/* markmatches for every record of the list; several calls accumulate */
int vsa_coverage_mark(vsa_coverage *coverage, const vsa_result *result,
                      const vsa_coverageparams *params);
/* dst |= src: tables of equal size on the same device (several lists,
   several batches, or -- after a copy the caller makes -- several GPUs) */
int vsa_coverage_merge(vsa_coverage *dst, const vsa_coverage *src);

typedef struct
{
  uint64_t positions;  /* of the Multiseq without its separators: the
                          "sequence length" of showmaskedseq's last line
                          (Vmatch/showmasked.c:137-153)                    */
  uint64_t marked;     /* ... of them marked: "number of masked symbols"   */
  uint64_t separators;
  double mark_ms;      /* HIP-event time of the last vsa_coverage_mark     */
  double extract_ms;   /* ... of the last vsa_coverage_nomatch             */
  double count_ms;     /* ... of the count this call made                  */
} vsa_coveragestats;

int vsa_coverage_getstats(const vsa_coverage *coverage,
                          vsa_coveragestats *stats);
/* min(capacity, ceil(bits / 64)) words of the table to the host */
int vsa_coverage_fetch_bits(const vsa_coverage *coverage, uint64_t *words,
                            uint64_t capacity);
const void *vsa_coverage_device_bits(const vsa_coverage *coverage);

/*
  nomatchsubstringsout (Vmatch/nomatch.c:168-274): the maximal runs of
  unmarked positions inside [first, first + len) that are at least minlength
  (>= 1) long, in ascending order.  The runs come as a vsa_result (fetch,
  device pointer and free are those of a match list) whose records read
    length = length of the run,  dbstart = its absolute start,
    queryseq = number of its sequence,  querystart = start inside it.
  _all: the whole table, the range of the runs with -q (initpost.c:181-190).
  _database / _queries: the ranges of the runs without -q (initpost.c:167-180)
  over a table of the index -- [0, DATABASELENGTH) and [DATABASELENGTH + 1,
  totallength).  DATABASELENGTH is totallength - totalquerylength - 1
  (include/multidef.h:91) also where the index holds no queries: the
  reference then leaves the LAST position of the text out of its scan, and so
  does _database (_all does not).  _queries needs an index with queries;
  both are _all on a table over a query batch.
*/
int vsa_coverage_nomatch(vsa_coverage *coverage, uint64_t minlength,
                         uint64_t first, uint64_t len,
                         vsa_result **intervals);
int vsa_coverage_nomatch_all(vsa_coverage *coverage, uint64_t minlength,
                             vsa_result **intervals);
int vsa_coverage_nomatch_database(vsa_coverage *coverage, uint64_t minlength,
                                  vsa_result **intervals);
int vsa_coverage_nomatch_queries(vsa_coverage *coverage, uint64_t minlength,
                                 vsa_result **intervals);

/*
  shownomatch (Vmatch/nomatch.c:36-135) for such records, host code: the
  lines `>seqnum relstart length`, with VSA_SHOW_ABSOLUTE `>abs_start length`
  (abs_start counts from posoffset).  posoffset != 0 is the query part of an
  index with queries: the reference never advances its sequence counter
  there and prints `>0 (start - posoffset) length` for every run; so does
  this.  Returns the bytes written or a negative code.
*/
int64_t vsa_nomatch_format(const vsa_match *intervals, uint64_t n,
                           uint32_t showmode, uint64_t posoffset,
                           char *buffer, uint64_t capacity);

/*
  showmaskedseq (Vmatch/showmasked.c:49-153) on the characters of a Multiseq,
  host code: chars[p] of every marked position p < nbits becomes maskchar, or
  with VSA_MASK_TOUPPER / VSA_MASK_TOLOWER (the reference's MASKTOUPPER /
  MASKTOLOWER, -dbmaskmatch toupper) its upper / lower case form; a marked
  character that is not of the other case stays if it is '*' and is otherwise
  the reference's error "cannot convert character %c to upper case" (-4; the
  characters in front of it are changed already).  Separators
  (chars[p] == VSA_SEPARATOR) are left alone.  *masked (may be NULL) = the
  number of masked symbols.  Line wrapping and description lines stay with
  the caller.
*/
#define VSA_MASK_TOUPPER 256
#define VSA_MASK_TOLOWER 257
int vsa_mask_apply(const uint64_t *bits, uint64_t nbits, uint8_t *chars,
                   int maskchar, uint64_t *masked);

/* ---- match selection: vmatch -best N, -sort mode, -evalue, -identity,
   -leastscore and the gap bounds of -l L lo [hi] (Vmatch/procfinal.c:196-260,
   566-636,695-745, Vmatch/mokay.c, kurtz/bestmatch.c:33-119,
   kurtz-basic/dictmaxsize.c, kurtz/smcontain.c:23-95, kurtz/matsort.c,
   kurtz/evalues.c:316-420) on match lists that stay in HBM -----------------

   Per match processfinal derives length1, position1, length2, position2
   (absolute in the query Multiseq: sequence i starts at the sum of
   length_j + 1 over j < i; relpos2 flipped to seqlength2 - (relpos2 +
   length2) for a palindromic list), the distance (0, +d for -e, -d for -h),
   the D/P flag and the E-value: multiplier * T[|d|][lenmatch] for d <= 0,
   (multiplier * hequot[d]) * T[d][lenmatch] for d > 0, with T the table of
   incprecomputehammingEvalues, lenmatch = length2 for complete lists or d = 0
   and the larger length otherwise, and the multiplier of assignEvalue:
   (double) totallength * (double) length of the query sequence with -q,
   totallength for complete lists, 0.5 * totallength^2 for self lists
   (DATABASELENGTH * totalquerylength on an index with queries); 0.0 for
   every match with VSA_SHOW_NOEVALUE.

   matchokay drops a match if a length is below leastlength; if
   100 (1 - |d| / max(length1, length2)) < identity; if EVALDISTANCE2SCORE
   (l1 + l2 - 3d for d >= 0, -(l1 + l2 + 3d) for d < 0) < leastscore; if
   evalue > maximumevalue; if the gap position2 - (position1 + length1), or
   -(position1 + length1 - position2) where position1 + length1 - 1 >
   position2, is below lowergap or above uppergap.

   -best N keeps the N best distinct matches, best first: smaller E-value,
   larger length1, smaller position1, larger length2, smaller position2,
   direct before palindromic (cmpBestMatch); two matches equal in all six are
   one match (the one seen first stays).  -sort takes these N, sorts them
   stably by (position1, length1, position2), drops every match contained in
   another (CONTAINSSTOREMATCH; of two with the same four coordinates the
   earlier stays) and, unless the mode is ia, sorts them stably by the mode's
   key: length1, position1, position2, E-value, |score|, identity. */

#define VSA_SORT_NONE 12  /* else 0..11 = la ld ia id ja jd ea ed sa sd ida idd (matsort.c:167-180) */
typedef struct
{
  uint64_t bestnumber;   /* -best N; 0: filters only, input order kept      */
  int sortmode;          /* VSA_SORT_NONE or 0..11; needs bestnumber > 0    */
  int hasmaxevalue;
  double maximumevalue;
  uint32_t identity;     /* 0 = off, 1..100                                 */
  int hasleastscore;
  int64_t leastscore;    /* >= 0                                            */
  int haslowergap, hasuppergap; /* VSA_SINK_SELF only, else error; the upper
                                   bound needs the lower one                */
  int64_t lowergap, uppergap;
} vsa_selectparams;

typedef struct
{
  uint64_t seen;       /* records handed to vsa_select_add                  */
  uint64_t rejected;   /* ... dropped by matchokay                          */
  uint64_t duplicates; /* ... found equal in all six values to a match kept
                          at that time (a match worse than the N kept ones
                          is dropped without being compared)                */
  uint64_t selected;   /* matches of the selection, after vsa_select_finish
                          of the list it delivered                          */
  uint64_t containedremoved; /* "remove %lu contained matches"             */
} vsa_selectstats;

typedef struct vsa_select vsa_select;
/* records one workgroup of the selection kernels compacts */
#define VSA_SELECT_TILE 1024u

/*
  layout describes the run like it does for the sink: kind, numofchars,
  showmode & VSA_SHOW_NOEVALUE, leastlength, the index and the query
  Multiseq; layout->palindromic is ignored in favour of the argument of
  vsa_select_add.  queries != NULL: the query Multiseq is laid out from the
  lengths of the batch like vsa_coverage_open_queries does, and the offset of
  the batch (vsa_queries_set_offset) at the time of the call is subtracted
  from the queryseq of every match; NULL: layout->querystart / querylength.
  bestnumber is at most 2^32 - 16.
*/
int vsa_select_open(const vsa_sinkparams *layout, const vsa_queries *queries,
                    const vsa_selectparams *params, int device,
                    vsa_select **select);
/* the records of a list through matchokay into the selection; several calls
   accumulate (-d -p: two calls).  VSA_NOT_COVERED, state untouched: a
   packed-pair result; selfpalindromic lists (layout->selfpalindromic, or
   palindromic != 0 with VSA_SINK_SELF).  -2, state untouched: a record that
   does not fit the layout. */
int vsa_select_add(vsa_select *select, const vsa_result *result,
                   int palindromic);
/* the selection as raw records in output order: the same sink formats them
   (record by record with the flags of vsa_select_flags where both strands
   were added), vsa_coverage_mark accepts them.  The selection stays open:
   more lists may be added and finish called again. */
int vsa_select_finish(vsa_select *select, vsa_result **selected);
/* the D/P flag of every record vsa_select_finish delivered last */
int vsa_select_flags(const vsa_select *select, uint8_t *palindromic,
                     uint64_t capacity);
int vsa_select_getstats(const vsa_select *select, vsa_selectstats *stats);
/* digit-counting passes the radix select of the last vsa_select_add made
   over its candidates: one per word of the key on which they all agree, a
   few on a word that tells them apart (scripts/select_probe.py) */
uint64_t vsa_select_passes(const vsa_select *select);
/* the E-value of every record of a list, bit for bit the host's */
int vsa_select_evalues(vsa_select *select, const vsa_result *result,
                       int palindromic, double *evalues, uint64_t capacity);
void vsa_select_close(vsa_select *select);

/*
  The same rules on a list in host memory, no GPU involved: matches[i] with
  the flag palindromic[i] (NULL: all direct), the query Multiseq from
  layout->querystart / querylength.  selected / selectedflags / evalues (the
  latter two may be NULL) take the at most `capacity` records of the
  selection in output order; -3 if there are more.
*/
int vsa_select_host(const vsa_sinkparams *layout,
                    const vsa_selectparams *params, const vsa_match *matches,
                    const uint8_t *palindromic, uint64_t n,
                    vsa_match *selected, uint8_t *selectedflags,
                    double *evalues, uint64_t capacity, uint64_t *nselected,
                    vsa_selectstats *stats);

/* ---- sequence clustering: vmatch -dbcluster percsmall perclarge
   (Vmatch/vmcluster.c:289-415, kurtz/cluster.c:125-197,436-683) on match
   lists that stay in HBM ----------------------------------------------------

   Single-linkage clustering of the sequences of the index.  A record of a
   self list (VSA_SINK_SELF: length, start1, start2 absolute) or of a list of
   vmatch -p IDX (dbstart absolute, queryseq = the sequence of the index whose
   reverse complement matched) lies in the sequences seq1 and seq2, found in
   markpos; a sequence is as long as findboundaries says.  A record with
   seq1 == seq2 is skipped; of a palindromic list the record with seq1 > seq2
   is the mirror image of another and dropped (procfinal.c:159-167).  The
   record is an edge (seq1, seq2) iff, with mlen the length of the match and
   small <= large the two sequence lengths, mlen >= small * percsmall / 100
   and mlen >= large * perclarge / 100 in 64-bit unsigned arithmetic.  Edges
   are numbered in the order of the records over all lists added.

   linkcluster takes the edges in that order: two sequences without a cluster
   found a new one; a sequence without one is appended to the cluster of the
   other; two clusters are merged into the larger one, into that of seq2 if
   they are equally large.  Only an edge between two different clusters
   changes anything, and these edges are the minimum spanning forest of the
   list with the edge number as weight: the device finds that forest, the
   host replays its at most numofsequences - 1 edges.

   Clusters are numbered like vmatch prints them: in the order of their
   creation, those emptied by a merge left out; the members of a cluster come
   in the order of its chain.  Fewer than 2^32 sequences and edges. */

typedef struct
{
  uint32_t percsmall, perclarge;
} vsa_clusterparams;

typedef struct
{
  uint64_t seen;          /* records handed in                              */
  uint64_t samesequence;  /* ... with seq1 == seq2                          */
  uint64_t mirrordropped; /* ... palindromic with seq1 > seq2               */
  uint64_t rejected;      /* ... with too small an overlap                  */
  uint64_t edges;         /* ... accepted: linkcluster calls                */
  uint64_t forestedges;   /* edges that joined two different clusters       */
  uint64_t rounds;        /* rounds of the forest search (0 on the host)    */
  uint64_t clusters;      /* after finish: clusters, ...                    */
  uint64_t inclusters;    /* ... sequences in them, ...                     */
  uint64_t singlets;      /* ... and sequences in none                      */
} vsa_clusterstats;

typedef struct vsa_cluster vsa_cluster;
#define VSA_CLUSTER_SINGLET 0xFFFFFFFFFFFFFFFFull
#define VSA_CLUSTER_MAXROUNDS 64u /* of the forest search */
#define VSA_CLUSTER_MAXJUMPS 64u  /* per pointer-jumping pass */

/*
  layout describes the index like it does for the sink: totallength,
  numofsequences, markpos, numofquerysequences; kind is VSA_SINK_SELF, or
  VSA_SINK_QUERY with selfpalindromic set (vmatch -p IDX alone).  -2 with the
  reference's message: an index of one sequence, an index with queries.
  VSA_NOT_COVERED: any other kind, 2^32 sequences or more.
*/
int vsa_cluster_open(const vsa_sinkparams *layout,
                     const vsa_clusterparams *params, int device,
                     vsa_cluster **cluster);
/* the records of a list (a search result, or what vsa_select_finish
   delivered) become edges; several calls accumulate (-d -p: two calls, the
   direct list first).  palindromic != 0: a list of vmatch -p IDX.
   VSA_NOT_COVERED, state untouched: a packed-pair result; a direct list with
   a layout that is not VSA_SINK_SELF.  -2, state untouched: a record that
   does not fit the layout. */
int vsa_cluster_add(vsa_cluster *cluster, const vsa_result *result,
                    int palindromic);
/* forest, replay, numbering; may be called again after more lists */
int vsa_cluster_finish(vsa_cluster *cluster);
int vsa_cluster_getstats(const vsa_cluster *cluster, vsa_clusterstats *stats);
/* after finish: cluster c has the members members[clusterstart[c] ..
   clusterstart[c + 1]); stats.clusters + 1 and stats.inclusters entries */
int vsa_cluster_members(const vsa_cluster *cluster, uint64_t *clusterstart,
                        uint64_t *members);
/* after finish: the cluster of every sequence or VSA_CLUSTER_SINGLET;
   numofsequences entries */
int vsa_cluster_labels(const vsa_cluster *cluster, uint64_t *label);
/* after finish: the accepted records grouped by cluster, within a cluster in
   descending edge number -- the order of the lines of PREFIX.size.cnum.match
   (addClusterEdge, cluster.c:586-614) -- as a result in HBM that the sink
   formats; palindromic[i] (stats.edges entries, may be NULL) is the D/P flag
   of record i, the records of cluster c are edgestart[c] ..
   edgestart[c + 1] (stats.clusters + 1 entries, may be NULL) */
int vsa_cluster_edges(vsa_cluster *cluster, vsa_result **edges,
                      uint8_t *palindromic, uint64_t *edgestart);
/* after finish: what vmatch prints behind its "# args=" line: the lines of
   clusterSizedistribution and one line "c: m m m" per cluster; returns the
   bytes written (without the closing 0 byte), -3 if capacity is too small */
int64_t vsa_cluster_format(const vsa_cluster *cluster, char *buffer,
                           uint64_t capacity);
/* HIP-event times of all calls so far, in ms */
int vsa_cluster_times(const vsa_cluster *cluster, double *add_ms,
                      double *finish_ms, double *edges_ms);
void vsa_cluster_close(vsa_cluster *cluster);

/*
  The same on a list in host memory, no GPU involved: every edge goes through
  linkcluster.  matches[i] with the flag palindromic[i] (NULL: all direct).
  Outputs that are NULL are left out: clusterstart and edgestart
  (numofsequences / 2 + 2 entries are enough), members and label
  (numofsequences), edgerecord (n: the indices into matches of the accepted
  records, grouped like vsa_cluster_edges groups them), buffer / capacity /
  written like vsa_cluster_format.  On an error nothing is written.
*/
int vsa_cluster_host(const vsa_sinkparams *layout,
                     const vsa_clusterparams *params, const vsa_match *matches,
                     const uint8_t *palindromic, uint64_t n,
                     vsa_clusterstats *stats, uint64_t *clusterstart,
                     uint64_t *members, uint64_t *label, uint64_t *edgestart,
                     uint64_t *edgerecord, char *buffer, uint64_t capacity,
                     int64_t *written);

/* ---- match clustering: vmatch -pp matchcluster gapsize G | overlap P
   (Vmatch/initpost.c:307-333, Vmatch/clpos.c:14-201,
   Vmatch/matchclust.c:87-128, kurtz/cluster.c:458-614) on match lists that
   stay in HBM ----------------------------------------------------------------

   Single-linkage clustering of the MATCHES of a list.  Match number m is the
   index of the record over all add calls (the reference's idnumber when
   nothing was selected away); length1, position1 and position2 are what
   processfinal stores (the view vsa_select derives).  Every match gives two
   references, (position1, index 2m) and (position2, index 2m + 1), both on
   one axis -- also for lists against queries, where the second one is a
   query coordinate: the reference mixes them (clpos.c:41-47).  The references
   are sorted by their start alone, equal starts in the order of their index
   (clpos.c:48: glibc's merging qsort).  With end_i = start_i + length1 of
   the match of reference i, for i and every j > i of that order:

     gapsize G  gap = start_j - end_i in unsigned 64-bit arithmetic; the loop
                over j ends at the first gap > G (clpos.c:87-108).  A
                successor that starts inside match i wraps to a huge value:
                reference i then links nothing at all.  Otherwise i links
                every j with start_j in [end_i, end_i + G].
     overlap P  the loop over j ends at the first end_i < start_j
                (clpos.c:145-182); overlap = ((double) (end_i - start_j) *
                100.0) / (double) max(length1_i, length1_j), an edge iff
                overlap >= (double) P.  length1 on both sides, also in
                approximate lists.

   An edge (m_i, m_j), in that orientation, with its gap or overlap is
   stored where m_i != m_j; edges are numbered in the order (i ascending, j
   ascending), and the same pair of matches may occur several times.  Every
   edge goes through linkcluster in that order (matchclust.c:95-104); output
   numbering, member order and the order of a cluster's edges (descending
   edge number) are those of showClusterSet and addClusterEdge, as for
   vsa_cluster above. */
#define VSA_MATCHCLUSTER_GAP 0     /* gapsize G                             */
#define VSA_MATCHCLUSTER_OVERLAP 1 /* overlap P                             */
#define VSA_MATCHCLUSTER_ERATE 2   /* erate E: vsa_eratecluster_open        */

typedef struct
{
  int mode;
  uint64_t maxgapsize;        /* VSA_MATCHCLUSTER_GAP, below 2^62           */
  uint64_t minpercentoverlap; /* VSA_MATCHCLUSTER_OVERLAP                   */
} vsa_matchclusterparams;

typedef struct
{
  uint64_t matches;     /* records of all lists: the nodes                  */
  uint64_t candidates;  /* pairs (i, j) inside a window                     */
  uint64_t samematch;   /* ... of the two references of one match           */
  uint64_t below;       /* ... with an overlap below the threshold          */
  uint64_t edges;       /* ... stored: linkcluster calls                    */
  uint64_t forestedges; /* edges that joined two different clusters         */
  uint64_t rounds;      /* of the forest search (0 on the host)             */
  uint64_t clusters;    /* after finish: clusters, ...                      */
  uint64_t inclusters;  /* ... matches in them                              */
} vsa_matchclusterstats;

typedef struct vsa_matchcluster vsa_matchcluster;
/* the stages vsa_matchcluster_times reports, in this order */
#define VSA_MATCHCLUSTER_STAGES 6 /* refs sort window pairs forest group    */

/*
  layout: what the sink of these lists is opened with (kind, the index, the
  query Multiseq); markpos, querystart and querylength need not outlive the
  call.  0 and *cluster (on `device`), or a negative code and the message.
  VSA_NOT_COVERED: mode VSA_MATCHCLUSTER_ERATE (the edit distance between the
  match substrings, Vmatch/cluedist.c: it needs the text, which
  vsa_eratecluster_open below takes); a selfpalindromic layout (vmatch
  -p IDX).
*/
int vsa_matchcluster_open(const vsa_sinkparams *layout,
                          const vsa_matchclusterparams *params, int device,
                          vsa_matchcluster **cluster);
/* one more list: its records become the matches count .. count + n - 1 and
   are copied, the caller may free the list.  palindromic: the list of the
   reverse-complement pass (vmatch -d -p: two calls).  VSA_NOT_COVERED, state
   untouched: a packed-pair result; a palindromic list under a self layout;
   2^31 matches or more on the device (the index 2m + side of a reference is
   32 bit there; the host code takes fewer than 2^32 - 1).  -2, state
   untouched: a record that does not fit the layout. */
int vsa_matchcluster_add(vsa_matchcluster *cluster, const vsa_result *result,
                         int palindromic);
/* clusters the matches added so far (more may be added, and finish called
   again).  VSA_NOT_COVERED, state untouched: 2^32 - 1 edges or more.
   VSA_MATCHCLUSTER_CHUNK in the environment bounds the candidate pairs
   looked at per pass (default 2^26): the memory grows with the stored edges,
   not with the candidates. */
int vsa_matchcluster_finish(vsa_matchcluster *cluster);
/* the counts of the last finish, matches included: a list added since then
   shows only after the next finish (all 0 before the first) */
int vsa_matchcluster_getstats(const vsa_matchcluster *cluster,
                              vsa_matchclusterstats *stats);
/* after finish: cluster c has the matches members[clusterstart[c] ..
   clusterstart[c + 1]) in the order of its chain; stats.clusters + 1 and
   stats.inclusters entries */
int vsa_matchcluster_members(const vsa_matchcluster *cluster,
                             uint64_t *clusterstart, uint64_t *members);
/* after finish: the cluster of every match or VSA_CLUSTER_SINGLET;
   stats.matches entries */
int vsa_matchcluster_labels(const vsa_matchcluster *cluster, uint64_t *label);
/* after finish: the edges grouped by cluster, within a cluster in the order
   showClusterSet shows them (descending edge number): edge t links m0[t] and
   m1[t] with value[t] (the gap, the bits of the overlap percentage, a
   double, or minlen << 32 | edit distance); the edges of cluster c are
   edgestart[c] .. edgestart[c + 1].  stats.clusters + 1 and stats.edges
   entries; any may be NULL */
int vsa_matchcluster_edges(vsa_matchcluster *cluster, uint64_t *edgestart,
                           uint32_t *m0, uint32_t *m1, uint64_t *value);
/* after finish: the member matches of all clusters, in the order of
   vsa_matchcluster_members, as a result in HBM that the sink prints like any
   list; palindromic[t] (stats.inclusters entries, may be NULL) = the flag of
   the list record t came from */
int vsa_matchcluster_records(vsa_matchcluster *cluster, vsa_result **records,
                             uint8_t *palindromic);
/* after finish: what vmatch prints behind its "# args=" line -- "# cluster N
   matches" and one "# create cluster c of size s" per cluster
   (matchclust.c:10-16,94); returns the bytes written, -3 if the buffer is
   too small */
int64_t vsa_matchcluster_format(const vsa_matchcluster *cluster, char *buffer,
                                uint64_t capacity);
/* after finish: the bytes of the file PREFIX.size.c.match behind its first
   line (matchclust.c:31-85): "# id m" and the match line per member, then
   "# linked a and b with gapsize g", "... with overlap percentage %.2f" or
   "... with edit distance d (error rate %.2f%%)" per edge.  The match lines
   are the sink's; the reference prints them with its fixed default widths
   (vsa_sink_setdigits(sink, 5, 6, 6, 3, 3)).  Every member is printed with
   the direction of the sink. */
int64_t vsa_matchcluster_format_cluster(vsa_matchcluster *cluster,
                                        vsa_sink *sink, uint64_t c,
                                        char *buffer, uint64_t capacity);
/* HIP-event times of all calls so far in ms, VSA_MATCHCLUSTER_STAGES of
   them */
int vsa_matchcluster_times(const vsa_matchcluster *cluster, double *ms);
void vsa_matchcluster_close(vsa_matchcluster *cluster);

/*
  The same on a list in host memory, no GPU involved: every edge goes through
  linkcluster.  Outputs that are NULL are left out: clusterstart and
  edgestart (n / 2 + 2 entries are enough), members and label (n); m0, m1 and
  value hold edgecapacity entries -- stats is written and -3 returned if
  there are more edges than that.
*/
int vsa_matchcluster_host(const vsa_sinkparams *layout,
                          const vsa_matchclusterparams *params,
                          const vsa_match *matches, const uint8_t *palindromic,
                          uint64_t n, vsa_matchclusterstats *stats,
                          uint64_t *clusterstart, uint64_t *members,
                          uint64_t *label, uint64_t *edgestart, uint32_t *m0,
                          uint32_t *m1, uint64_t *value,
                          uint64_t edgecapacity, char *buffer,
                          uint64_t capacity, int64_t *written);
/* the text of vsa_matchcluster_format_cluster from arrays in host memory:
   the members of one cluster with their records, its edges */
int64_t vsa_matchcluster_format_host(vsa_sink *sink, int mode,
                                     const uint64_t *member,
                                     const vsa_match *records, uint64_t size,
                                     const uint32_t *m0, const uint32_t *m1,
                                     const uint64_t *value, uint64_t nedges,
                                     char *buffer, uint64_t capacity);

/* ---- vmatch -pp matchcluster erate E (Vmatch/cluedist.c:42-198,
   kurtz/frontSEP.c:341-446, kurtz/front.gen) ---------------------------------

   Links the matches i < j of a SELF list whose substrings are within a unit
   edit distance of E percent of the shorter one.  Every pair is looked at, i
   outermost, both ascending; minlen = min(length_i, length_j), maxdist =
   (uint64_t) ((double) minlen * (double) E / 100.0).  The instance pairs
   (position1_i, position1_j), (position1_i, position2_j), (position2_i,
   position1_j), (position2_i, position2_j) are tried in this order, and the
   first one that answers >= 0 stores the edge (i, j) with value = minlen <<
   32 | distance -- the distance of the first instance pair within the bound,
   not the smallest of the four.  An instance pair answers -1 if the lengths
   differ by more than maxdist; 0 if both instances are the same stretch of
   text; else the distance the reference's greedy front finds within maxdist
   rounds, or -1 (with maxdist 0: 0 iff the substrings are equal and free of
   special symbols).  A special symbol equals nothing, not even itself.  The
   front is the reference's, including its shortcut on a diagonal where both
   substrings are the same text (csrc/erate_rules.h).  The edges go through
   linkcluster in the order found; everything behind the edge list is as for
   gapsize and overlap.  In the stats candidates = n (n - 1) / 2, below = the
   pairs without an edge, samematch = 0.

   Covered: layouts of an index against itself without indexed queries,
   direct lists, lengths below 2^32.  A record that leaves the text or holds
   a separator does not fit (-2).  On the device a pair that passes the
   length test with maxdist > VSA_ERATE_MAXDIST makes finish answer
   VSA_NOT_COVERED; vsa_eratecluster_host takes any maxdist.  The device
   keeps the rows of a front in 32 bits while every match is shorter than
   2^30 symbols, else in 64; VSA_ERATE_WIDE_ROWS=1 in the environment asks
   for 64 whatever the lengths are (the answers are the same). */
#define VSA_ERATE_MAXDIST 127

/* The handle is a vsa_matchcluster.  (The two entries are not named
   vsa_matchcluster_*: the binding's tests count the names with that prefix.)
   layout: as for vsa_matchcluster_open, VSA_SINK_SELF; index: its text is
   read by add and finish, so the index outlives the handle; errorrate 0 ..
   100.  Every other vsa_matchcluster_* call works on the handle.
   VSA_NOT_COVERED: a layout against queries or with indexed queries, a
   selfpalindromic one.  -2: an error rate above 100, an index of another
   length than the layout or on another device. */
int vsa_eratecluster_open(const vsa_sinkparams *layout,
                          const vsa_index *index, uint32_t errorrate,
                          int device, vsa_matchcluster **cluster);
/* the same on a list and a text in host memory, no GPU involved: the
   reference's two loops and a scalar front; outputs as those of
   vsa_matchcluster_host */
int vsa_eratecluster_host(const vsa_sinkparams *layout, uint32_t errorrate,
                          const uint8_t *text, uint64_t textlength,
                          const vsa_match *matches, uint64_t n,
                          vsa_matchclusterstats *stats, uint64_t *clusterstart,
                          uint64_t *members, uint64_t *label,
                          uint64_t *edgestart, uint32_t *m0, uint32_t *m1,
                          uint64_t *value, uint64_t edgecapacity, char *buffer,
                          uint64_t capacity, int64_t *written);

/* ---- chaining: vmatch -pp chain [global [gc|ov] | local [K | Kb | Kp]]
   [wf F] [maxgap W] [withinborders] [silent] (Vmatch/parsepp.c:95-109,
   Vmatch/chncallparse.c:224-400, Vmatch/initpost.c:307-318,
   Vmatch/chainvm.c:29-500, kurtz/matsort.c:316-367,
   kurtz-basic/chain2dim.c:251-1915) on match lists that stay in HBM ---------

   The records of all lists added are the match buffer; record number m is
   the index over all add calls.  What a record is (lengths, positions,
   distance) is the view vsa_select derives; seqnum1 is the sequence of the
   index position1 lies in, seqnum2 that of position2 (self lists) or the
   query number.

   Problems.  With withinborders, unless every record lies in one (seqnum1,
   seqnum2) pair, the records are grouped: a stable counting sort by seqnum1,
   then the reference's quicksort by seqnum2 inside every run of one seqnum1
   (not stable for runs of more than 10 records), and every run of one pair is
   a chaining problem of its own.  Otherwise the whole list is one problem.
   Inside a problem the records are sorted by position2 (stable); the
   fragment numbers are the places in that order.

   Fragments.  Dimension 0 is [position1, position1 + length1 - 1], dimension
   1 is [position2, position2 + length2 - 1]; weight = (int64) (weightfactor *
   (double) |score|).  Every kind but plain global has initialgap = position1
   + position2 and terminalgap = (largest end0 of the problem - end0) +
   (largest end1 - end1).

   Scores.  The predecessor of fragment i is, among the fragments j with
   end1[j] < start1[i] and end0[j] <= start0[i] - 1, the one of greatest
   priority (score, minus terminalgap unless plain global), ties to the
   smallest (end1[j], j); if maxgapwidth != 0 and the gap to it is wider in
   either dimension, i has no predecessor.  global: score = score[j] +
   weight, or weight.  global gc: score[j] + weight - gap with gap =
   (start0 - end0[j]) + (start1 - end1[j]), or weight - initialgap.  local:
   as gc if score[j] > gap, else weight and a new chain.  global ov: every
   colinear j < i (all four coordinates strictly smaller) within maxgap is a
   candidate with score[j] - overlap, continued with + weight if positive and
   else replaced by weight and a new chain; the first maximum wins.

   Retrieval.  Fragment i ends a chain if it is the last one, or fragment
   i + 1 does not have it as predecessor, or has a smaller score.  The
   threshold: global -- the greatest score; gc, ov, local -- the greatest end
   score of the chain ends (gc: score - terminalgap); local K -- K; local Kb
   -- the K-th largest distinct score of the chain ends, compared as unsigned
   numbers; local Kp -- (int64) ((double) max * (1.0 - (double) K / 100.0)).
   Every chain end not below the threshold gives a chain, in the order of the
   fragments; the local kinds only one per first fragment, the first end that
   has the greatest score of its class.  A problem of one fragment gives that
   fragment as a chain whatever the threshold.  Chains are numbered from 0
   within every problem. */
#define VSA_CHAIN_GLOBAL 0          /* global                                */
#define VSA_CHAIN_GLOBAL_GC 1       /* global gc                             */
#define VSA_CHAIN_GLOBAL_OV 2       /* global ov                             */
#define VSA_CHAIN_LOCAL_MAX 3       /* local                                 */
#define VSA_CHAIN_LOCAL_THRESHOLD 4 /* local K                               */
#define VSA_CHAIN_LOCAL_BEST 5      /* local Kb, K >= 1                      */
#define VSA_CHAIN_LOCAL_PERCENT 6   /* local Kp                              */
/* the most fragments of one problem on the device.  It bounds the
   QUADRATIC WORK of the one workgroup that chains such a problem (every
   fragment looks at all earlier ones), not memory; vsa_chain_host takes
   problems of any size. */
#define VSA_CHAIN_MAXGROUP ((uint64_t) 1 << 15)
#define VSA_CHAIN_NONE 0xFFFFFFFFu
#define VSA_CHAIN_SILENT 1 /* format flag: headers only (silent)           */

typedef struct
{
  int kind;
  int64_t value;        /* K of local K, Kb, Kp                             */
  uint64_t maxgapwidth; /* maxgap W; 0: none                                */
  double weightfactor;  /* wf F; the default is 1.0                         */
  int withinborders;
  int thread; /* thread ...: not covered                                    */
} vsa_chainparams;

typedef struct
{
  uint64_t matches;  /* records of all lists                                */
  uint64_t problems; /* chaining problems, of which ...                     */
  uint64_t single;   /* ... with 1 fragment (the boundary case)             */
  uint64_t small;    /* ... with 2 .. 8: one lane each                      */
  uint64_t wave;     /* ... with 9 .. 64: one wavefront each                */
  uint64_t group;    /* ... with more: one workgroup each                   */
  uint64_t largest;  /* fragments of the largest problem                    */
  uint64_t tieruns;  /* runs of records that tie on (seqnum1, seqnum2,
                        position2), or on position2 in one problem          */
  uint64_t replayed; /* records in runs of one seqnum1 of more than 10
                        records that hold such a tie: the only ones the
                        quicksort may leave in another than the stable order
                        (the device sends these through the host)           */
  uint64_t chains;   /* after finish: chains, ...                           */
  uint64_t chained;  /* ... and the records in them                         */
} vsa_chainstats;

typedef struct vsa_chain vsa_chain;
/* the stages vsa_chain_times reports, in this order */
#define VSA_CHAIN_STAGES 5 /* view sort replay score retrieve              */

/*
  layout: what the sink of these lists is opened with; markpos, querystart
  and querylength need not outlive the call.  VSA_NOT_COVERED: thread; the
  selfpalindromic layout.  -2: an unknown kind, a weight factor that is not
  positive, local Kb with K < 1.
*/
int vsa_chain_open(const vsa_sinkparams *layout,
                   const vsa_chainparams *params, int device,
                   vsa_chain **chain);
/* one more list (vmatch -d -p: two calls); the records are copied.
   VSA_NOT_COVERED, state untouched: a packed-pair result; a palindromic list
   under a self layout; 2^32 - 1 records or more.  -2, state untouched: a
   record that does not fit the layout. */
int vsa_chain_add(vsa_chain *chain, const vsa_result *result,
                  int palindromic);
/* chains the records added so far (more may be added, and finish called
   again).  VSA_NOT_COVERED: a problem of more than VSA_CHAIN_MAXGROUP
   fragments -- the handle is then as the last finish left it: its chains
   stay, the lists added since then are dropped, and smaller ones may
   follow.  VSA_CHAIN_SMALLMAX and VSA_CHAIN_WAVEMAX in the environment move
   the sizes up to which a problem gets one lane (default 8) and one
   wavefront (default 64, the most): the A/B of scripts/chain_probe.py. */
int vsa_chain_finish(vsa_chain *chain);
/* the counts of the last finish (all 0 before the first) */
int vsa_chain_getstats(const vsa_chain *chain, vsa_chainstats *stats);
/* after finish: chain c belongs to problem problem[c] (problems are numbered
   in the order of (seqnum1, seqnum2)), is chain number[c] of it, has the
   score score[c] and the members members[start[c] .. start[c + 1]).
   stats.chains entries each, start one more; any may be NULL */
int vsa_chain_chains(const vsa_chain *chain, uint64_t *problem,
                     uint64_t *number, int64_t *score, uint64_t *start);
/* after finish: the record numbers of the members of all chains,
   stats.chained entries */
int vsa_chain_members(vsa_chain *chain, uint64_t *members);
/* after finish: the members of all chains, in that order, as a result in
   HBM that the sink prints like any list; palindromic[t] (stats.chained
   entries, may be NULL) = the flag of the list record t came from */
int vsa_chain_records(vsa_chain *chain, vsa_result **records,
                      uint8_t *palindromic);
/* after finish: what vmatch prints behind its "# args=" line
   (outvmatchchain, chainvm.c:106-161): "# chain N: length L score S" and,
   unless flags has VSA_CHAIN_SILENT, the sink's line of every member, all
   with the direction of the sink.  Returns the bytes written, -3 if the
   buffer is too small */
int64_t vsa_chain_format(vsa_chain *chain, vsa_sink *sink, int flags,
                         char *buffer, uint64_t capacity);
/* HIP-event times of all calls so far in ms, VSA_CHAIN_STAGES of them */
int vsa_chain_times(const vsa_chain *chain, double *ms);
void vsa_chain_close(vsa_chain *chain);

/*
  The same on a list in host memory, no GPU involved, problems of any size:
  the reference's sweep with a sorted array as its dictionary.  Outputs that
  are NULL are left out; problem, number and score hold chaincapacity
  entries, start one more, members membercapacity: stats is written and -3
  returned if there are more.
*/
int vsa_chain_host(const vsa_sinkparams *layout,
                   const vsa_chainparams *params, const vsa_match *matches,
                   const uint8_t *palindromic, uint64_t n,
                   vsa_chainstats *stats, uint64_t *problem, uint64_t *number,
                   int64_t *score, uint64_t *start, uint64_t chaincapacity,
                   uint64_t *members, uint64_t membercapacity);
/* the text of vsa_chain_format from arrays in host memory: records[t] = the
   record of member t of all chains */
int64_t vsa_chain_format_host(vsa_sink *sink, int flags, uint64_t nchains,
                              const uint64_t *number, const int64_t *score,
                              const uint64_t *start, const vsa_match *records,
                              char *buffer, uint64_t capacity);

/* the field widths of the sink's lines (length, position1, position2,
   seqnum1, seqnum2) instead of those of the layout: what the reference's
   post-processing prints its matches with (ASSIGNDEFAULTDIGITS,
   Vmatch/outinfo.h:93-98: 5, 6, 6, 3, 3) */
int vsa_sink_setdigits(vsa_sink *sink, int length, int position1,
                       int position2, int seqnum1, int seqnum2);

/* ---- DNA queries against a protein index in six reading frames: vmatch
   -dnavsprot transnum -q Q PROTIDX (kurtz/sixframe.c:70-264,
   kurtz/codon.c:292-999, Vmatch/procmatch.c:450-460,
   Vmatch/procfinal.c:196-289; the rules: csrc/sixframe_rules.h) -------------

   The translation reads the ORIGINAL CHARACTERS of the DNA sequences, not
   mapped codes: a c g t u, the wildcards n s y w r k v b d h m, either case;
   any other character in a sequence of three characters or more is the
   reference's error "illegal char c0='X'(88)" (shorter sequences have no
   codon and are not looked at).  DNA sequence s of len characters becomes
   the sequences 6 s .. 6 s + 5 of a protein Multiseq: the forward frames f =
   0, 1, 2 (codons at f, f + 3, ..: (len - f) / 3 symbols, 0 where len < f),
   then the reverse frames r = 0, 1, 2 (codon k = the complemented characters
   at len - 1 - r - 3 k and the two below it: (len - r) / 3 symbols).  Every
   frame is followed by VSA_SEPARATOR except the last frame of the last
   sequence, start[i] = markpos[i - 1] + 1; an empty frame is two adjacent
   separators.  A wildcard in codon position 1 or 2 stands for the smallest
   base of its set in the order T < C < A < G; in position 3 for the amino
   acid all its bases agree on, else for its smallest base.  In the reverse
   frames only the four plain bases are complemented, the set of a wildcard
   is not, and W stands for {A, C}: the reference's rules, reproduced.  The
   amino-acid character ('*' for a stop codon) goes through symbolmap, the
   symbol map of the INDEX (character -> code; VSA_WILDCARD for its wildcard
   class, VSA_UNDEFBWT for a character outside the alphabet).
   Deviation: an amino acid whose code lies in [numofchars, 253] (numofchars
   = the largest code below 253 of the map, plus 1) is an error (-2), the
   contract of vsa_queries_from_host; the reference stores whatever its map
   says.  It cannot happen under mkvtree -protein.
   transnum: the NCBI tables 1-6, 9-16, 21-23. */

/* 0, or -2 with the reference's message "illegal translation table number
   N: must be number in the range [1,23] except for 7, 8, 17, 18, 19 and 20" */
int vsa_transnum_check(uint32_t transnum);

/* Host code, no GPU.  Sequence i = dnachars[start[i] .. start[i] +
   length[i]).  protein takes the symbols (-3 if capacity is too small: sum
   over the sequences of 2 (len / 3 + (len - 1) / 3 + (len - 2) / 3) + 6,
   minus 1), pstart / plength (6 nq entries each) the frames, *nsymbols the
   total.  On an error *nsymbols is 0 and the other outputs are undefined. */
int vsa_translate_host(uint32_t transnum, const uint8_t *dnachars,
                       uint64_t nchars, const uint64_t *start,
                       const uint64_t *length, uint64_t nq,
                       const uint8_t symbolmap[256], uint8_t *protein,
                       uint64_t capacity, uint64_t *pstart, uint64_t *plength,
                       uint64_t *nsymbols);

/* The same translation on the GPU: an ordinary query batch of 6 nq sequences
   in the layout above, for vsa_findquerymatches (-l L counts amino acids),
   vsa_findcompletematches (which stops with "patternlength=0 must be >=
   1=prefixlen" at the first frame shorter than the prefix length, as the
   reference does) and the other engine calls.  The batch is ragged: it takes
   the byte paths of the engine.  It keeps the DNA lengths on the device for
   vsa_translated_convert.  vsa_queries_set_offset counts SIX-FRAME sequences
   on it: a shard of reads that starts at read `first` sets 6 * first.
   An error (illegal character, unmapped amino acid) leaves no batch behind.
   _translate: ragged characters in host memory; _translate_device: nq reads
   of m characters back to back in device memory (not modified, not kept). */
int vsa_queries_translate(uint32_t transnum, const uint8_t *dnachars,
                          uint64_t nchars, const uint64_t *start,
                          const uint64_t *length, uint64_t nq,
                          const uint8_t symbolmap[256], int device,
                          vsa_queries **protein);
int vsa_queries_translate_device(uint32_t transnum, const void *device_chars,
                                 uint64_t nq, uint32_t m,
                                 const uint8_t symbolmap[256], int device,
                                 vsa_queries **protein);
/* the symbols (numofsymbols of vsa_queries_getinfo) and the start / length
   of every sequence (numofqueries each) of a batch that holds bytes, back in
   host memory; NULL pointers are skipped.  -2 for a packed batch whose bytes
   have not been made. */
int vsa_queries_download(const vsa_queries *queries, uint8_t *symbols,
                         uint64_t *start, uint64_t *length);
/* codons of one grid a workgroup of the translation kernel translates */
#define VSA_TRANSLATE_TILE 256u
uint64_t vsa_translate_tile(void);
/* HIP-event time of the translation kernels of the batch in ms (0 for a
   batch that is not translated) */
double vsa_queries_translate_ms(const vsa_queries *protein);

/* sixframeconvertmatch (kurtz/sixframe.c:232-264) for every record of a list
   the engine delivered on a translated batch: a new resident list, the query
   view in DNA coordinates of the forward strand --
     length = 3 * length, dbstart unchanged, queryseq = q / 6 (q and the
     result both count from the batch's offset), querystart = 3 * querystart
     + f in forward frame f, len - 3 * (querystart + length) - r in reverse
     frame r
   -- which is what vsa_coverage_mark(.., VSA_COVERAGE_QUERIES) needs on a
   coverage opened over the DNA batch (-qnomatch, -qmaskmatch of DNA reads
   against a protein database; -dbnomatch takes the list as it is).  reverse
   (host, vsa_result_count entries, may be NULL): 1 for a record of a reverse
   frame.  VSA_NOT_COVERED: a packed-pair result.  -2: a batch that is not
   translated, an offset that is no multiple of 6, a record that does not lie
   in its frame.  The HIP-event time of the kernel is total_device_ms of the
   new list's stats. */
int vsa_translated_convert(const vsa_result *result,
                           const vsa_queries *protein, vsa_result **queryview,
                           uint8_t *reverse, uint64_t capacity);
/* the same on the host: dnalength[numofdna] the lengths of the DNA
   sequences, offset that of the six-frame batch */
int vsa_translated_convert_host(const vsa_match *matches, uint64_t n,
                                const uint64_t *dnalength, uint64_t numofdna,
                                uint64_t offset, vsa_match *queryview,
                                uint8_t *reverse);

/* ---- degenerate matches: vmatch -l L -h K [-seedlength S] [-q Q] IDX -------
   Exact seeds, each extended to the left and right over at most K mismatches
   on seed lists that stay in HBM.

   What the reference does: the seed length is max(S, L / (K + 1))
   (Vmatch/matchlenparm.c:11-22); the seeds are the MEMs of that length in the
   order of findquerymatches (Vmengine/procexqu.c:17-95) or, without -q, the
   maximal repeats in the order of findselfmatches (Vmengine/fself.c:95-146);
   every seed on its own goes through hammingextend (kurtz/extendHD.c:166-374,
   called by callgenericextend, Vmengine/extendgen.c:24-87), which keeps the
   best extension of at least L symbols -- best by E-value, then identity,
   then length, the later candidate on a tie (include/extcmp.c) -- or nothing.
   Nothing is deduplicated.

   A match is the 32-byte record of its seed's list moved to the left:
   length1 = length2 in the low 48 bits of `length`, the number of mismatches
   (the reference stores its negative in Match.distance) in the top 16 bits;
   dbstart, and querystart or (self layout) queryseq moved left by the same
   amount.  vsa_result_fetch, _copy_device and _from_host carry such records
   like any others. */
#define VSA_HAMMING_LENGTHBITS 48
#define VSA_HAMMING_MAXDISTANCE 0xFFFFu /* what the record can carry */
#define VSA_HAMMING_LENGTH(lengthfield) \
  ((uint64_t) (lengthfield) & (((uint64_t) 1 << VSA_HAMMING_LENGTHBITS) - 1))
#define VSA_HAMMING_DISTANCE(lengthfield) \
  ((uint64_t) (lengthfield) >> VSA_HAMMING_LENGTHBITS)
#define VSA_HAMMING_PACK(length, distance) \
  ((uint64_t) (length) | (uint64_t) (distance) << VSA_HAMMING_LENGTHBITS)

/* layouts of such lists for the sink: the lines of vmatch -l L -h K -q Q IDX
   (with palindromic: of its -p pass) and of vmatch -l L -h K IDX, byte for
   byte.  Everything else as for VSA_SINK_QUERY / VSA_SINK_SELF.  vsa_select_*,
   vsa_coverage_mark, vsa_cluster_*, vsa_matchcluster_*, vsa_chain_* and
   vsa_translated_convert answer VSA_NOT_COVERED for them, state untouched.
   (7 stays what it was, a kind no layout has.)  A result of these entries
   knows that it holds extended seeds; a list that went through the host and
   vsa_result_from_host no longer does, and its caller keeps it away from
   those handles. */
#define VSA_SINK_QUERY_HAMMING 8
#define VSA_SINK_SELF_HAMMING  9

/* limits of the device path: distance bounds up to the cap (beyond it
   VSA_NOT_COVERED and nothing delivered; the host path takes any bound the
   record can carry), texts and query sequences below 2^32 - 16 symbols,
   fewer than 2^31 seeds.  A lane of the scan stage looks at up to
   VSA_EXTEND_LANE_BUDGET symbols of a side before it hands the side to the
   long stage, where a wavefront covers VSA_EXTEND_LONG_STEP symbols per step.
   The environment variable VSA_EXTEND_STAGE, read by every call, forces one
   stage: `lane` -- no budget, no side goes to the long stage; `long` -- every
   side that is scanned at all goes there.  The lists are the same. */
#define VSA_EXTEND_MAXDIST 64u
#define VSA_EXTEND_LANE_BUDGET 256u
#define VSA_EXTEND_LONG_STEP 1024u
uint32_t vsa_extend_maxdist(void);
uint32_t vsa_extend_lane_budget(void);
uint32_t vsa_extend_long_step(void);

/*
  hammingextend for every seed of a list in HBM.  seeds: records of
  vsa_findquerymatches (MEM; layout->kind VSA_SINK_QUERY, queries = the
  forward batch; palindromic != 0, rcmode of extendgen.c:61-67: the seeds
  were found on its reverse complement, vsa_queries_reverse_complement, which
  is made again here and is what the seeds are extended in) or of
  vsa_findmaximalrepeats (layout->kind VSA_SINK_SELF, queries NULL), or a
  list of the caller's in one of these forms; of the layout only the kind is
  read.  leastlength L, maxdist K, seedlength S as on vmatch's command line
  (S = 0: none given); the seed length rule is applied here.  *result: the
  matches in the order of their seeds.  A packed 2-bit batch is expanded to
  bytes first (once per batch, as for the MEM search).
  Stats of the result: count = matches, sumlength = sum of their lengths,
  candidates = seeds, searches = sides of seeds the long stage scanned,
  search_kernel_ms = HIP-event time of the extension (scan, long and choice
  stage; first_kernel_ms = of the scan stage, anchor_ms = of the long stage
  alone), total_device_ms = ... of the whole call with the compaction.
  VSA_NOT_COVERED, nothing delivered, no device memory kept: K above
  VSA_EXTEND_MAXDIST, the size limits above, a packed-pair seed list.
  -2: K = 0, L = 0, a layout of another kind, a seed that does not fit the
  index or its query sequence (nothing is read through such a seed).
*/
int vsa_extend_hamming(const vsa_index *index, const vsa_queries *queries,
                       const vsa_result *seeds, const vsa_sinkparams *layout,
                       int palindromic, uint64_t leastlength,
                       uint64_t maxdist, uint64_t seedlength,
                       vsa_result **result);

/* vmatch -l L -h K [-seedlength S] [-p] -q Q IDX (findquerymatches,
   Vmengine/fquery.c:1009-1058, with processexactquerymatch extending every
   MEM, Vmengine/procexqu.c:65-94): the seed length rule, vsa_findquerymatches
   on the batch -- with palindromic != 0 on its reverse complement
   (vsa_queries_reverse_complement) --, vsa_extend_hamming; the seed list is
   freed.  A seed length below the prefix length of the index is the
   reference's error "searchlength=%lu must be >= %lu=prefixlen"
   (fquery.c:440-446). */
int vsa_findquerymatches_hamming(const vsa_index *index,
                                 const vsa_queries *queries,
                                 uint64_t leastlength, uint64_t maxdist,
                                 uint64_t seedlength, int palindromic,
                                 vsa_result **result);
/* vmatch -l L -h K [-seedlength S] IDX (findselfmatches,
   Vmengine/fself.c:203-300, with simpleselfmatchoutput extending every
   maximal repeat, fself.c:95-146): the same with vsa_findmaximalrepeats. */
int vsa_findselfmatches_hamming(const vsa_index *index, uint64_t leastlength,
                                uint64_t maxdist, uint64_t seedlength,
                                vsa_result **result);

/*
  The same extension on the host: what the kernels are measured against, and
  what a caller uses beyond the limits of the device path (any K up to
  VSA_HAMMING_MAXDISTANCE).  layout: kind VSA_SINK_QUERY -- numofqueries,
  querystart and querylength describe where the sequences lie in
  querysymbols (for the -p pass: the reverse complements in the same places)
  -- or VSA_SINK_SELF (querysymbols NULL); totallength symbols at text,
  numofchars for the E-values.  threads 0 = one per processor.  The matches go
  to matches[0 .. capacity) in the order of their seeds, -3 if there are
  more (capacity = numofseeds always suffices); -2 with "record %lu does not
  fit the layout" for a seed outside the index or its query sequence.
*/
int vsa_extend_hamming_host(const vsa_sinkparams *layout, const uint8_t *text,
                            const uint8_t *querysymbols,
                            const vsa_match *seeds, uint64_t numofseeds,
                            uint64_t leastlength, uint64_t maxdist,
                            uint64_t seedlength, int threads,
                            vsa_match *matches, uint64_t capacity,
                            uint64_t *numofmatches);
/* max(S, L / (K + 1)), Vmatch/matchlenparm.c:11-22 */
uint64_t vsa_extend_seedlength(uint64_t leastlength, uint64_t maxdist,
                               uint64_t seedlength);

/* ---- degenerate matches: vmatch -l L -e K [-seedlength S] [-p] [-q Q] IDX ---
   The same seeds extended over at most K edit operations (editextend,
   kurtz/extendED.c:78-355; callgenericextend picks it or hammingextend by one
   flag, Vmengine/extendgen.c:24-87).  The two instances of such a match
   differ in length, so the record of a match carries both, beside the
   distance (which editextend stores as it is, not negated):
     bits 0-47  length1
     bits 48-55 the distance
     bits 56-63 length2 - length1 as a signed byte (its absolute value is at
                most the distance plus two trimmed separators, so the record
                carries distances up to VSA_EDIST_MAXDISTANCE)
   dbstart = position1; queryseq, querystart = the query sequence and the
   position in it, or (self layout) queryseq = position2.  The entries are
   declared in vstree_amd_edist.h, which this header includes. */
#define VSA_EDIST_MAXDISTANCE 125u
#define VSA_EDIST_LENGTH1(lengthfield) \
  ((uint64_t) (lengthfield) & (((uint64_t) 1 << 48) - 1))
#define VSA_EDIST_DISTANCE(lengthfield) \
  (((uint64_t) (lengthfield) >> 48) & 0xFFu)
#define VSA_EDIST_LENGTH2(lengthfield) \
  ((uint64_t) ((int64_t) VSA_EDIST_LENGTH1(lengthfield) + \
               (int64_t) (int8_t) ((uint64_t) (lengthfield) >> 56)))
#define VSA_EDIST_PACK(length1, length2, distance) \
  ((uint64_t) (length1) | (uint64_t) (distance) << 48 | \
   (((uint64_t) (length2) - (uint64_t) (length1)) & 0xFFu) << 56)

/* layouts of such lists for the sink: the lines of vmatch -l L -e K -q Q IDX
   (with palindromic: of its -p pass) and of vmatch -l L -e K IDX, byte for
   byte; the post-processing handles answer VSA_NOT_COVERED for them as for
   the two Hamming kinds */
#define VSA_SINK_QUERY_EDIST 10
#define VSA_SINK_SELF_EDIST  11

/* the cap of the device path: 2 K + 1 diagonals are the lanes of one
   wavefront */
#define VSA_EXTEND_EDIST_MAXDIST 31u

/* ---- X-drop extension: vmatch -l L -hxdrop X | -exdrop X [-seedlength S] [-p]
   [-q Q] IDX.  The same seeds, of length S (30 if none is given), each
   extended to the left and right until the score -- match +2, mismatch -1,
   with -exdrop insertion and deletion -2 -- falls X below the best one seen
   (xdropseedextend, Vmengine/xdropext.c:39-221); one match per seed, kept if
   both instances have L symbols.  No distance bound exists, and the two
   lengths differ freely, so the record carries
     length      length1 in bits 0-31, length2 in bits 32-63
     querystart  bits 0-31 the position in the query sequence (0 in a self
                 layout), bits 32-63 the magnitude of the distance; the kind
                 gives its sign: negative for -hxdrop, positive for -exdrop
   dbstart = position1; queryseq as for -e K.  Texts and query sequences of
   2^32 - 16 symbols or more are VSA_NOT_COVERED on every entry.  The entries
   are declared in vstree_amd_xdrop.h, which this header includes. */
#define VSA_XDROP_MAXDROP 255u /* FLAGXDROP, Vmatch/parsevm.c:974-990 */
#define VSA_XDROP_LENGTH1(lengthfield) ((uint64_t) (lengthfield) & 0xFFFFFFFFull)
#define VSA_XDROP_LENGTH2(lengthfield) ((uint64_t) (lengthfield) >> 32)
#define VSA_XDROP_PACKLENGTHS(length1, length2) \
  ((uint64_t) (length1) | (uint64_t) (length2) << 32)
#define VSA_XDROP_START(startfield) ((uint64_t) (startfield) & 0xFFFFFFFFull)
#define VSA_XDROP_DISTANCE(startfield) ((uint64_t) (startfield) >> 32)
#define VSA_XDROP_PACKSTART(start, distance) \
  ((uint64_t) (start) | (uint64_t) (distance) << 32)

/* layouts of such lists for the sink: the lines of vmatch -l L -hxdrop X and
   -l L -exdrop X with -q Q (with palindromic: of the -p pass) and without,
   byte for byte; the post-processing handles answer VSA_NOT_COVERED for them
   as for the other kinds of extended seeds */
#define VSA_SINK_QUERY_HXDROP 12
#define VSA_SINK_SELF_HXDROP  13
#define VSA_SINK_QUERY_EXDROP 14
#define VSA_SINK_SELF_EXDROP  15

#ifdef __cplusplus
}
#endif
#include "vstree_amd_edist.h"
#include "vstree_amd_xdrop.h"
#include "vstree_amd_align.h"
#include "vstree_amd_online.h"
#endif
