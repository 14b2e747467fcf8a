// Query matching on MI355X (vmatch -complete | -l L | -mum [cand] -q Q IDX):
// kernels (in the .inc files below) and their host-side pipelines.  DESIGN.md has the byte
// budgets and the measurements.
//
//   search_complete.inc  K1  k_complete_search   one work-item per query:
//                            locate -> lcptab widening -> suffix-array
//                            interval [left, left+count)
//                            k_complete_expand   one workgroup per 256 queries
//   search_query.inc     K2  k_query_search      one work-item per (query,
//                            offset): locate -> MEM enumeration or
//                            MUM-candidate test; wavefront-aggregated append
//                            into sharded regions, compaction, stable radix
//                            sort by work-item number = reference order
//   mum_workplan.inc     K2a k_mum_first / k_mum_plan: which offsets of a read
//                            can be MUM candidates at all; K2 in its planned
//                            forms: k_mum_walk_tiles (MUM: wavefronts that
//                            take tiles of planned reads from a queue) and
//                            k_query_search_planned (MEM; VSA_TUNE=32)
//   mem_workplan.inc     K2m k_repeat_bits / k_mem_plan: which offsets of a
//                            read a MEM search has to look at
//   candidate_sort.inc   K4s candidates as (sort key, value) pairs thrown
//                            into buckets by the high bits of dbstart from
//                            where they were produced, every bucket sorted
//                            and filtered in LDS by K4's rule, the survivors
//                            written as records in order (short or
//                            concentrated lists: compaction, rocPRIM's radix
//                            sort and K4)
//   mum_filter.inc       K4  one filter on sorted (key, value) pairs, in
//                            tiles: running maximum of the right ends, flags
//                            from the keys, survivors written as records in
//                            order (kurtz/cleanMUMcand.c:55-118).  Two
//                            sorts in front of it: rocPRIM on dbstart alone
//                            (runs of equal dbstarts looked at as runs),
//                            rocPRIM on all bits (a run too long for that;
//                            candidate records, as composite key + index)
// The other families have translation units of their own since round 4:
//   selfmum_search.hip       K3, the scan over an index that holds its queries
//   approx_entry.hip         -complete -e/-h (approx_search.inc, approx_tree.inc)
//   selfmatch_entry.hip      maximal / supermaximal / tandem repeats
//   candidate_partition.hip  grouping of MUM candidates for the N > 1 form
//   index_derive.hip         the derived tables (esa8, slot16, tis2)
//   search_common.hip        what they share (search_host.hpp)
//
// rocPRIM supplies radix sort / scan / reduce only.
//
// Host side: run_complete (K1), and run_query (K2 with its plans, K4) as
// stages over one QueryRun -- work-items, decisions, the MEM or the MUM plan,
// the search, compaction, the result.  pickform() picks the form of every
// search launch (Form: reference walk, deep, staged, rows, windows) and
// withform() turns it into template arguments; RecordForm is how matches
// travel; query_entry() is what the four C entries share.
//
// Switches (environment, read when an index is created):
//   VSA_TUNE=2        no work reduction: every offset of every read is
//                     searched by the list form of the search kernel (the
//                     cross-check of first pass + work plan)
//   VSA_TUNE=4        MUM candidates sorted by rocPRIM's radix sort whatever
//                     their number (A/B and cross-check of the bucket sort)
//   VSA_TUNE=8        ... by the bucket sort whatever their number (tests on
//                     small texts; by default lists below VSA_CS_MINPAIRS
//                     take rocPRIM)
//   VSA_TUNE=16       no walk in the planned MUM search: every planned offset
//                     is located, one per work-item (A/B and cross-check of
//                     the walk, mum_workplan.inc)
//   VSA_TUNE=32       the planned MUM search through the workgroup tiles of
//                     k_query_search_planned: a lane keeps one chunk per pass
//                     (A/B and cross-check of the tile queue,
//                     k_mum_walk_tiles)
//                     (a bit mask: 2, 4, 8, 16 and 32 combine)
//   VSA_WALK_CHUNK=N  offsets of a plan range that one lane walks (a power of
//                     two, else the next one below; default 8; 1 is
//                     VSA_TUNE=16: every planned offset a work-item of its
//                     own)
//   VSA_WALK_GRID=N   workgroups of the tile queue (default 0: as many as the
//                     device holds at once; for tests and probes: 1 makes four
//                     wavefronts take every tile)
//   VSA_NO_ESA8=1     no deep tables: the reference walk, probe for probe
//   VSA_DEEP_PREFIX=D their depth (default ceil(log4 n), at most 16)
//   VSA_FORCE_WIDE=1  64-bit device tables whatever the size of the text
// What was measured and dropped is described in DESIGN.md section 4.
#include "search_host.hpp"
#include <rocprim/rocprim.hpp>
#include <type_traits>

#include "search_complete.inc"
#include "search_query.inc"
#include "mum_workplan.inc"
#include "mem_workplan.inc"
#include "mum_filter.inc"
#include "candidate_sort.inc"
#include <atomic>

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

namespace
{

// ---- launch forms ----

// How a search launch reads its queries and the index: the template
// arguments <DEEP, PQ, ROWS, WINDOWS> of k_complete_search and k_mum_first
enum class Form
{
  Ref,    // the reference walk: no deep tables
  Deep,   // deep tables, queries as bytes
  Staged, // deep tables, reads of one length m (a multiple of 4, <= 128)
          // back to back, staged through LDS and packed
  Rows,   // deep tables, packed rows of up to four words whole in registers
  Windows // deep tables, rows of up to eight words through windows of the row
};

// the launches a form is picked for
enum class Stage
{
  Complete, // k_complete_search
  MemFirst, // k_mum_first in front of the MEM plan
  MumFirst, // k_mum_first in front of the MUM plan (and the plan and the
            // planned search behind it)
  Bytes     // the MEM plan's search and every search without a plan
};

Form pickform(const vsa_index *index, const vsa_queries *queries,
              const DevQueries &qs, Stage stage, uint32_t searchlength)
{
  // (-complete: a query shorter than D takes the walk of the deep kernel;
  // everywhere else the deep prefix has to fit into every search)
  const bool deep = index->esa8 != nullptr &&
                    (stage == Stage::Complete || searchlength >= index->D);
  bool rows = queries->rows != nullptr && queries->roww <= 8;
  bool staged = qs.dense != 0 && qs.uniformlen <= 128 &&
                (qs.uniformlen & 3u) == 0;
  switch (stage)
  {
  case Stage::Complete:
    // the row and the staged kernel locate D symbols of every read (staging
    // copies the bytes into LDS)
    rows = rows && queries->maxlength >= index->D;
    staged = staged && qs.symbols != nullptr && qs.uniformlen >= index->D;
    break;
  case Stage::MemFirst: // rows, though the MEM search behind it reads bytes
  case Stage::MumFirst: // (asked for only under the MUM work reduction)
    break;
  case Stage::Bytes: // bytes, made from the rows by vsa_queries_bytes
    rows = staged = false;
    break;
  }
  if (!deep)
  {
    return Form::Ref;
  }
  if (rows)
  {
    return queries->roww > 4 ? Form::Windows : Form::Rows;
  }
  return staged ? Form::Staged : Form::Deep;
}

// fn(DEEP, PQ, ROWS, WINDOWS) with std::integral_constant<bool> arguments
template <typename Fn>
void withform(Form form, Fn &&fn)
{
  using T = std::true_type;
  using F = std::false_type;
  switch (form)
  {
  case Form::Ref:
    return fn(F(), F(), F(), F());
  case Form::Deep:
    return fn(T(), F(), F(), F());
  case Form::Staged:
    return fn(T(), T(), F(), F());
  case Form::Rows:
    return fn(T(), T(), T(), F());
  case Form::Windows:
    return fn(T(), T(), T(), T());
  }
}

// dynamic LDS of a launch: the staged reads of a workgroup
size_t ldsbytes(Form form, const DevQueries &qs)
{
  return form == Form::Staged ? (size_t) VSA_BLOCK * qs.uniformlen : 0;
}

// ---- K1 pipeline ----

template <typename IDX>
int run_complete(const vsa_index *index, const vsa_queries *queries,
                 uint64_t qlimit, vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  // packed batches: read from their rows by the deep kernel (whole in
  // registers up to four words, through windows up to eight); an index
  // without deep tables, or longer reads, takes their bytes
  if (queries->rows != nullptr &&
      pickform(index, queries, devqueries(queries), Stage::Complete, 0) <
          Form::Rows &&
      vsa_queries_bytes(queries, stream) != 0)
  {
    return -100;
  }
  const DevQueries qs = devqueries(queries);
  const Form form = pickform(index, queries, qs, Stage::Complete, 0);
  DevBuf left, count, offsets, matches;
  uint64_t total = 0;

  res->stats.searches = qlimit;
  if (qlimit == 0)
  {
    return 0;
  }
  if (left.alloc(qlimit * 8) || count.alloc((qlimit + 1) * 8) ||
      offsets.alloc((qlimit + 1) * 8))
  {
    return -100;
  }
  tall.start();
  VSA_HIP(hipMemsetAsync(count.as<uint64_t>() + qlimit, 0, 8, stream));
  tsearch.start();
  withform(form, [&](auto deep, auto pq, auto rows, auto windows) {
    k_complete_search<IDX, deep, pq, rows, windows>
        <<<gridfor(qlimit), VSA_BLOCK, ldsbytes(form, qs), stream>>>(
            ix, qs, qlimit, left.as<uint64_t>(), count.as<uint64_t>());
  });
  tsearch.stop();
  VSA_HIP(hipGetLastError());
  if (exclusive_sum(count.as<uint64_t>(), offsets.as<uint64_t>(), qlimit,
                    stream, &total))
  {
    return -100;
  }
  if (total > 0)
  {
    if (matches.alloc(total * sizeof(vsa_match)))
    {
      return -100;
    }
    k_complete_expand<IDX><<<gridfor(qlimit), VSA_BLOCK, 0, stream>>>(
        ix, qs, qlimit, left.as<uint64_t>(), offsets.as<uint64_t>(), total,
        matches.as<vsa_match>());
    VSA_HIP(hipGetLastError());
  }
  // (every complete match has the length of its query)
  return finish(res, matches, total, tall, tsearch, stream);
}

// ---- K2 (+K4) pipeline ----

// MUM candidates, any order -> MUMs in dbstart order
// (max dbstart, max length) of a candidate list
struct MaxPair
{
  uint64_t db, len;
};

struct MaxPairOf
{
  __device__ MaxPair operator()(const vsa_match &m) const
  {
    MaxPair p;
    p.db = m.dbstart;
    p.len = m.length;
    return p;
  }
};

struct MaxPairOp
{
  __device__ MaxPair operator()(const MaxPair &a, const MaxPair &b) const
  {
    MaxPair p;
    p.db = a.db > b.db ? a.db : b.db;
    p.len = a.len > b.len ? a.len : b.len;
    return p;
  }
};

// one key for "dbstart ascending, then length descending"
__global__ void __launch_bounds__(VSA_BLOCK)
k_mum_compositekeys(const vsa_match *__restrict__ cand, uint64_t n,
                    unsigned int lenbits, uint64_t *__restrict__ key,
                    uint32_t *__restrict__ idx)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < n)
  {
    const uint64_t lenmask = (1ull << lenbits) - 1;
    key[i] = (cand[i].dbstart << lenbits) | (lenmask - cand[i].length);
    idx[i] = (uint32_t) i;
  }
}

// ---- K4: rocPRIM's sort, one filter (mum_filter.inc) ----

// What the sorter fills and the filter reads: the pairs in dbstart order, the
// flag word (device; bit 0: a run was too long for the filter by runs), the
// filter's tiles
struct SortedPairs
{
  DevBuf k2, v2, flag, keep, tmax, tcarry, tcount, toff, tsum, tsumscan;
  uint64_t n = 0, ntiles = 0;
  // the tiles and the room for the MUMs (all that sorted records need) ...
  int alloc_tiles(uint64_t ncand, DevBuf &mums)
  {
    n = ncand;
    ntiles = (ncand + VSA_FT_TILE - 1) / VSA_FT_TILE;
    return tmax.alloc((ntiles + 1) * 8) || tcarry.alloc((ntiles + 1) * 8) ||
           tcount.alloc((ntiles + 1) * 8) || toff.alloc((ntiles + 1) * 8) ||
           tsum.alloc((ntiles + 1) * 8) || tsumscan.alloc((ntiles + 1) * 8) ||
           keep.alloc(ntiles * VSA_FT_TILE) || flag.alloc(8) ||
           mums.alloc(ncand * sizeof(vsa_match));
  }
  // ... and the pairs
  int alloc(uint64_t ncand, size_t valbytes, DevBuf &mums)
  {
    return alloc_tiles(ncand, mums) || k2.alloc(ncand * 8) ||
           v2.alloc(ncand * valbytes);
  }
  template <typename WRITER>
  PackedCands<WRITER> pairs(unsigned int lenbits, WRITER write)
  {
    return {{k2.as<uint64_t>(), lenbits}, v2.as<typename WRITER::VAL>(), write};
  }
};

// number of MUMs, sum of their lengths, the flag word
struct MumCounts
{
  uint64_t nmums, sumlength, flags;
};

// The filter on the sorted candidates `cands` (a view of mum_filter.inc on
// the s.n candidates): SORTED = by dbstart and, inside a run, longest first,
// else by dbstart alone (then bit 0 of c->flags may come back up, and the
// MUMs are not to be used).  carry = the reference's running `dbright` when
// it reaches the first of these candidates: 0 for a whole job, the largest
// right end of all candidates with a smaller dbstart when the list is one
// dbstart range of a job that is filtered in pieces (multi-GPU).
template <bool SORTED, typename CANDS>
int mumfilter_tiles(SortedPairs &s, CANDS cands, uint64_t carry,
                    hipStream_t stream, DevBuf &mums, MumCounts *c)
{
  using Rule = typename CANDS::Rule;
  const dim3 tg = vsa_grid(s.ntiles);
  k_mumf_tilemax<Rule><<<tg, VSA_BLOCK, 0, stream>>>(cands, s.n,
                                                     s.tmax.as<uint64_t>());
  k_mumf_scan<1><<<1, VSA_BLOCK, 0, stream>>>(
      s.tmax.as<uint64_t>(), s.ntiles, carry, s.tcarry.as<uint64_t>());
  k_mumf_flags<SORTED, Rule><<<tg, VSA_BLOCK, 0, stream>>>(
      cands, s.n, s.tcarry.as<uint64_t>(), s.keep.as<uint8_t>(),
      s.tcount.as<uint64_t>(), s.tsum.as<uint64_t>(),
      s.flag.as<unsigned int>());
  // (offsets of the tiles and, in a second workgroup, the sum of the lengths)
  k_mumf_scan<0><<<2, VSA_BLOCK, 0, stream>>>(
      s.tcount.as<uint64_t>(), s.ntiles, 0, s.toff.as<uint64_t>(),
      s.tsum.as<uint64_t>(), s.tsumscan.as<uint64_t>());
  k_mumf_write<<<tg, VSA_BLOCK, 0, stream>>>(
      cands, s.keep.as<uint8_t>(), s.n, s.toff.as<uint64_t>(),
      mums.as<vsa_match>());
  VSA_HIP(hipGetLastError());
  const Fetch f[3] = {{s.toff.as<uint64_t>() + s.ntiles, 8},
                      {s.tsumscan.as<uint64_t>() + s.ntiles, 8},
                      {s.flag.p, 8}};
  uint64_t got[3];
  if (fetchwords(stream, f, 3, got))
  {
    return -100;
  }
  c->nmums = got[0];
  c->sumlength = got[1];
  c->flags = got[2];
  return 0;
}

// sorter: rocPRIM's radix sort on bits [firstbit, endbit) of the keys (and
// the flag word zeroed in front of it).
// keys_in / vals_in: anything rocPRIM can read (pointers, or iterators over
// rows of pairs as they come out of the exchange: no copy into two arrays)
template <typename VAL, typename KeyIn, typename ValIn>
int sort_radix(KeyIn keys_in, ValIn vals_in, SortedPairs &s,
               unsigned int firstbit, unsigned int endbit, hipStream_t stream)
{
  DevBuf temp;
  VSA_HIP(hipMemsetAsync(s.flag.p, 0, 8, stream));
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::radix_sort_pairs(p, tb, keys_in, s.k2.as<uint64_t>(),
                                     vals_in, s.v2.as<VAL>(), (size_t) s.n,
                                     firstbit, endbit, stream);
  }));
  return 0;
}

// MUMs of a packed candidate list: keys and values as PairRecord (rec) reads
// them (k_query_search with packbits), so the candidates never exist as
// 32-byte records.  Sorted by dbstart alone and filtered by runs; a run that
// is too long for that (or allbits: the caller knows of one) sends the list
// through the sort on all bits.
template <typename VAL, typename KeyIn, typename ValIn>
int mumfilter_packed(KeyIn keys_in, ValIn vals_in, uint64_t ncand,
                     PairRecord<VAL> rec, unsigned int dbbits, uint64_t carry,
                     bool allbits, hipStream_t stream, DevBuf &mums,
                     MumCounts *c)
{
  *c = MumCounts();
  if (ncand == 0)
  {
    return 0;
  }
  SortedPairs s;
  if (s.alloc(ncand, sizeof(VAL), mums))
  {
    return -100;
  }
  const unsigned int endbit = rec.lenbits + dbbits;
  if (!allbits)
  {
    if (sort_radix<VAL>(keys_in, vals_in, s, rec.lenbits, endbit, stream) ||
        mumfilter_tiles<false>(s, s.pairs(rec.lenbits, rec), carry, stream,
                               mums, c))
    {
      return -100;
    }
    allbits = (c->flags & 1u) != 0;
  }
  if (allbits &&
      (sort_radix<VAL>(keys_in, vals_in, s, 0, endbit, stream) ||
       mumfilter_tiles<true>(s, s.pairs(rec.lenbits, rec), carry, stream,
                             mums, c)))
  {
    return -100;
  }
  return 0;
}

// wide records (dbstart and length do not fit into one key, or 2^32
// candidates and more): least significant key first (length descending), then
// a stable sort by dbstart; the tiled filter on the sorted records
int mumfilter_wide(DevBuf &cand, uint64_t ncand, uint64_t carry,
                   hipStream_t stream, DevBuf &mums, MumCounts *c)
{
  SortedPairs s;
  DevBuf sorted, k1, k2, kout;
  if (s.alloc_tiles(ncand, mums) || k1.alloc(ncand * 8) ||
      k2.alloc(ncand * 8) || kout.alloc(ncand * 8) ||
      sorted.alloc(ncand * sizeof(vsa_match)))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(s.flag.p, 0, 8, stream));
  k_mum_keys<<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
      cand.as<vsa_match>(), ncand, k1.as<uint64_t>(), k2.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  if (sortbykey(k1.as<uint64_t>(), kout.as<uint64_t>(), cand.as<vsa_match>(),
                sorted.as<vsa_match>(), ncand, 64, stream))
  {
    return -100;
  }
  k_mum_keys<<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
      sorted.as<vsa_match>(), ncand, k1.as<uint64_t>(), k2.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  if (sortbykey(k2.as<uint64_t>(), kout.as<uint64_t>(),
                sorted.as<vsa_match>(), cand.as<vsa_match>(), ncand, 64,
                stream))
  {
    return -100;
  }
  return mumfilter_tiles<true>(s, RecordCands{cand.as<vsa_match>()}, carry,
                               stream, mums, c);
}

// MUMs of candidate records, any order.  carry: see mumfilter_tiles.
// dbbound / lenbound: upper bounds of dbstart and length if the caller knows
// them (index length, longest query), else 0: they are looked up.
// *sumlength = sum of the lengths of the MUMs.
int mumuniqueinquery(DevBuf &cand, uint64_t ncand, hipStream_t stream,
                     DevBuf &mums, uint64_t *nmums, uint64_t *sumlength,
                     uint64_t carry = 0, uint64_t dbbound = 0,
                     uint64_t lenbound = 0)
{
  *nmums = 0;
  *sumlength = 0;
  if (ncand == 0)
  {
    return 0;
  }
  // how many bits do dbstart and length need?
  MaxPair mx;
  mx.db = dbbound;
  mx.len = lenbound;
  if (dbbound == 0 || lenbound == 0)
  {
    DevBuf temp, dmax;
    if (dmax.alloc(sizeof(MaxPair)))
    {
      return -100;
    }
    auto in = rocprim::make_transform_iterator(cand.as<vsa_match>(),
                                               MaxPairOf());
    MaxPair init;
    init.db = init.len = 0;
    VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
      return rocprim::reduce(p, tb, in, dmax.as<MaxPair>(), init,
                             (size_t) ncand, MaxPairOp(), stream);
    }));
    VSA_HIP(hipMemcpyAsync(&mx, dmax.p, sizeof mx, hipMemcpyDeviceToHost,
                           stream));
    VSA_HIP(hipStreamSynchronize(stream));
  }
  const unsigned int lenbits = bitsfor(mx.len), dbbits = bitsfor(mx.db);
  MumCounts c;
  if (lenbits + dbbits > 64 || ncand >= 0xFFFFFFFFull)
  {
    if (mumfilter_wide(cand, ncand, carry, stream, mums, &c))
    {
      return -100;
    }
  } else
  {
    // sorter: (composite key, index) over just the bits in use; the pair
    // list of the records
    SortedPairs s;
    DevBuf k1, i1;
    if (s.alloc(ncand, 4, mums) || k1.alloc(ncand * 8) ||
        i1.alloc(ncand * 4))
    {
      return -100;
    }
    k_mum_compositekeys<<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
        cand.as<vsa_match>(), ncand, lenbits, k1.as<uint64_t>(),
        i1.as<uint32_t>());
    VSA_HIP(hipGetLastError());
    if (sort_radix<uint32_t>(k1.as<uint64_t>(), i1.as<uint32_t>(), s, 0,
                             lenbits + dbbits, stream) ||
        mumfilter_tiles<true>(
            s, s.pairs(lenbits, GatheredRecord{cand.as<vsa_match>()}), carry,
            stream, mums, &c))
    {
      return -100;
    }
  }
  *nmums = c.nmums;
  *sumlength = c.sumlength;
  return 0;
}

// How the matches of a call travel from the search kernels to the result:
// vsa_match records, or (MUM) 8-byte values queryseq << 16 | querystart
// next to keys dbstart << lenbits | (2^lenbits - 1 - length), see
// mumfilter_packed -- 4-byte values where query number and offset fit.
struct RecordForm
{
  bool keeppairs; // the result is the pairs (vsa_findmumcandidates_packed)
  bool packed;
  unsigned int lenbits, dbbits;
  uint32_t packbits, valbits; // as the kernels take them (0: not this form)
  size_t recsize;
};

// forcebits != 0 (with domumcand, !ordered): the candidates stay pairs with
// this many length bits
int recordform(const vsa_index *index, const vsa_queries *queries, bool domum,
               bool domumcand, bool ordered, uint32_t forcebits,
               RecordForm *rf)
{
  const unsigned int need = bitsfor(queries->maxlength);
  rf->keeppairs = domum && domumcand && !ordered && forcebits != 0;
  rf->lenbits = rf->keeppairs ? forcebits : need;
  rf->dbbits = bitsfor(index->n);
  rf->packed = domum && (!domumcand || rf->keeppairs) &&
               rf->lenbits + rf->dbbits <= 64 && rf->lenbits >= need &&
               queries->maxlength < 0xFFFFu &&
               ((queries->nq + queries->seqoffset) >> 48) == 0;
  if (rf->keeppairs && !rf->packed)
  {
    VSA_ERROR("packed candidates: %u length bits do not fit this batch "
              "(longest query %lu, index %lu)", forcebits,
              (unsigned long) queries->maxlength, (unsigned long) index->n);
    return -2;
  }
  rf->packbits = rf->packed ? rf->lenbits : 0;
  // (not for pairs that travel to other ranks: those carry the global query
  // number)
  const bool small = ((queries->nq << rf->lenbits) >> 32) == 0;
  rf->valbits = (rf->packed && !rf->keeppairs && small) ? rf->lenbits : 0;
  rf->recsize = rf->valbits != 0 ? 4 : (rf->packed ? 8 : sizeof(vsa_match));
  return 0;
}

// the filled part of every cursor region of raw / rawkeys (cap records
// each) into out / keys from record `at` on
int compact_into(const RecordForm &form, DevBuf &raw, DevBuf &rawkeys,
                 uint64_t cap, DevBuf &cursors, DevBuf &doff, DevBuf &out,
                 DevBuf &keys, uint64_t at, hipStream_t stream)
{
  auto launch = [&](auto rec) {
    using REC = decltype(rec);
    k_compact_shards<REC><<<VSA_CURSOR_SHARDS, VSA_BLOCK, 0, stream>>>(
        raw.as<REC>(), rawkeys.as<uint64_t>(), cap,
        cursors.as<unsigned long long>(), doff.as<uint64_t>(),
        out.as<REC>() + at, keys.as<uint64_t>() + at);
  };
  if (form.valbits != 0)
  {
    launch(uint32_t());
  } else if (form.packed)
  {
    launch(uint64_t());
  } else
  {
    launch(vsa_match());
  }
  VSA_HIP(hipGetLastError());
  return 0;
}

// what the stages of one run_query call share
struct QueryRun
{
  const vsa_index *index;
  const vsa_queries *queries;
  hipStream_t stream;
  DevQueries qs;
  bool domum, domumcand, ordered;
  uint32_t searchlength;
  RecordForm rec;
  Timer tall, tsearch, tfirst; // tfirst: the first pass kernel alone
  // work-items: perquery per query, or (ragged batches) base[q] in front of
  // query q (dbase)
  DevBuf base;
  const uint64_t *dbase = nullptr;
  uint32_t perquery = 0;
  uint64_t nitems = 0;
  bool reduce = false, memplan = false;
  // of the search kernel, and of the MUM first pass and plan
  Form form = Form::Ref;
  // first pass + work plan (mum_workplan.inc, mem_workplan.inc)
  DevBuf wcount, wtemp, wplan, wlist, wfirste, wfmlen, wfmdb, wboffset;
  // reads the first pass left to the plan (low half) | first-pass candidates
  // (high half), on the device
  const uint64_t *nlistword = nullptr;
  // the cursor regions the plan answers into (PlanEmit), if it does
  DevBuf pcursor, pdoff, psummary, prawout, prawkeys;
  uint64_t pcap = 0;
  bool fromplan = false, planemit = false;
  uint64_t plansearches = 0;
  // the search kernel's cursor regions, and the dense list behind them
  DevBuf cursor, doff, summary, blocksum, rtemp, rawout, rawkeys, out, keys;
  uint64_t shardcap = 0, needed = 0, nplan = 0, nfirst = 0, plannedwork = 0;
  uint64_t plannedlocates = 0; // of plannedwork offsets: located by the walk
  double searchms = 0;

  QueryRun(const vsa_index *ix, const vsa_queries *q, bool mum, bool cand,
           bool ord, uint32_t least)
      : index(ix), queries(q), stream(ix->stream), qs(devqueries(q)),
        domum(mum), domumcand(cand), ordered(ord), searchlength(least),
        tall(stream), tsearch(stream), tfirst(stream)
  {
  }
};

// work-items: one per query suffix with remaining >= searchlength
// (kurtz/matchsub.c:187-196: shorter queries are skipped silently)
// (IDX: one instance of the device lambda per offset width)
template <typename IDX>
int workitems(QueryRun &st)
{
  const uint64_t nqr = st.queries->nq, least = st.searchlength;
  if (st.qs.uniformlen != 0)
  {
    st.perquery = (st.qs.uniformlen >= least) ? st.qs.uniformlen - least + 1
                                              : 0;
    st.nitems = (uint64_t) st.perquery * nqr;
    return 0;
  }
  // base[q] = number of work-items in front of query q, from the lengths
  // on the device (a host loop and an upload of 8 bytes per query cost
  // more than the search for a batch of millions of reads)
  DevBuf btemp;
  auto items = rocprim::make_transform_iterator(
      rocprim::counting_iterator<uint64_t>(0),
      [len = st.qs.length, nqr, least] __device__(uint64_t q) -> uint64_t {
        if (q >= nqr)
        {
          return 0; // the entry behind the last query: the total
        }
        const uint64_t l = len[q];
        return l >= least ? l - least + 1 : 0;
      });
  if (st.base.alloc((nqr + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(rocprim_run(btemp, [&](void *p, size_t &tb) {
    return rocprim::exclusive_scan(p, tb, items, st.base.as<uint64_t>(),
                                   (uint64_t) 0, (size_t) (nqr + 1),
                                   rocprim::plus<uint64_t>(), st.stream);
  }));
  st.dbase = st.base.as<uint64_t>();
  const Fetch f = {st.dbase + nqr, 8};
  return fetchwords(st.stream, &f, 1, &st.nitems) ? -100 : 0;
}

// lcptab's quirk, the work reductions, the form of the search (and the
// bytes of a packed batch that is not read from its rows)
int decide(QueryRun &st)
{
  const vsa_index *index = st.index;
  const vsa_queries *queries = st.queries;
  // ragged batches take the same route with per-query geometry
  const uint64_t maxoffsets =
      (queries->maxlength >= st.searchlength)
          ? queries->maxlength - st.searchlength + 1
          : 0;
  if (st.domum && queries->maxlength >= 255 && index->lcpquirk < 0)
  {
    uint8_t b = 0;
    if (index->n >= 2)
    {
      VSA_HIP(hipMemcpyAsync(&b, index->lcp + index->n - 1, 1,
                             hipMemcpyDeviceToHost, st.stream));
      VSA_HIP(hipStreamSynchronize(st.stream));
    }
    index->lcpquirk = (b == 255) ? 1 : 0;
  }
  // VSA_TUNE=2: no work reduction (every offset is searched by the list form
  // of the search kernel -- the cross-check of first pass and work plan)
  const bool exhaustive = (index->tune & 2u) != 0;
  const bool planable = maxoffsets > 1 && maxoffsets < 0xFFFFu &&
                        queries->nq < 0xFFFFFFFFull && !exhaustive;
  // The MUM work reduction (see k_mum_first, k_mum_plan) rests on "a match
  // that is not unique is no candidate"; the reference's test for lcp >= 255
  // (fquery.c:352) breaks that rule in one situation, which one byte of
  // lcptab rules out (see vsa_index::lcpquirk).  A plan holds 16-bit offsets.
  st.reduce = st.domum && planable &&
              !(queries->maxlength >= 255 && index->lcpquirk != 0);
  // MEM (-l L): first pass, then the plan of mem_workplan.inc -- aligned
  // stretches answered from one bit per text position, the rest searched
  st.memplan = !st.domum && planable && index->esa8 != nullptr &&
               st.searchlength >= index->D && st.searchlength <= 255;
  // packed batches (reads at two bits per symbol): MUM under the work
  // reduction reads the rows in every kernel; everything else takes the
  // bytes, which are made on the device once per batch
  st.form = pickform(index, queries, st.qs,
                     st.reduce ? Stage::MumFirst : Stage::Bytes,
                     st.searchlength);
  if (queries->rows != nullptr && st.form < Form::Rows)
  {
    if (vsa_queries_bytes(queries, st.stream) != 0)
    {
      return -100;
    }
    st.qs = devqueries(queries);
  }
  return 0;
}

// k_mum_first over all reads, timed, behind the allocation of the buffers of
// first pass and plan; blockcount: see k_mum_first
template <typename IDX>
int first_pass(QueryRun &st, const DevIndex<IDX> &ix, Form form,
               uint64_t *blockcount)
{
  st.tfirst.start();
  withform(form, [&](auto deep, auto pq, auto rows, auto windows) {
    k_mum_first<IDX, deep, pq, rows, windows>
        <<<gridfor(st.queries->nq), VSA_BLOCK, ldsbytes(form, st.qs),
           st.stream>>>(ix, st.qs, st.perquery, st.searchlength,
                        st.wcount.as<uint32_t>(), st.wfirste.as<uint32_t>(),
                        st.wfmlen.as<uint32_t>(), st.wfmdb.as<uint64_t>(),
                        blockcount);
  });
  st.tfirst.stop();
  VSA_HIP(hipGetLastError());
  return 0;
}

// the buffers of first pass and plan
int alloc_first(QueryRun &st)
{
  const uint64_t nq = st.queries->nq;
  return st.wcount.alloc((nq + 1) * 4) || st.wfirste.alloc(nq * 4) ||
         st.wfmlen.alloc(nq * 4) || st.wfmdb.alloc(nq * 8) ||
         st.wplan.alloc(nq * sizeof(PlanRanges));
}

// The cursor regions a plan kernel answers into, with room for `rounds`
// answers per read of all the workgroups that share a region (no
// overflow); cursors zeroed.
int plan_emit(QueryRun &st, uint32_t rounds, PlanEmit *em)
{
  const uint32_t nshards = VSA_CURSOR_SHARDS;
  const uint64_t nb = blocksfor(st.queries->nq),
                 pershard = (nb + nshards - 1) / nshards;
  st.pcap = pershard * VSA_BLOCK * rounds;
  if (st.pcursor.alloc((size_t) nshards * VSA_CURSOR_STRIDE * 8) ||
      st.pdoff.alloc(nshards * 8) || st.psummary.alloc(4 * 8) ||
      st.prawout.alloc(nshards * st.pcap * st.rec.recsize) ||
      st.prawkeys.alloc(nshards * st.pcap * 8))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(st.pcursor.p, 0,
                         (size_t) nshards * VSA_CURSOR_STRIDE * 8, st.stream));
  em->base = st.dbase;
  em->perquery = st.perquery;
  em->out = st.prawout.as<vsa_match>();
  em->outkey = st.prawkeys.as<uint64_t>();
  em->shardcap = st.pcap;
  em->shardmask = nshards - 1;
  em->cursors = st.pcursor.as<unsigned long long>();
  em->packbits = st.rec.packbits;
  em->valbits = st.rec.valbits;
  st.planemit = true;
  return 0;
}

// the counts of the plan's cursor regions, where each goes in the list
hipError_t plan_summary(QueryRun &st)
{
  return shard_summary(st.pcursor.as<unsigned long long>(), VSA_CURSOR_SHARDS,
                       st.pdoff.as<uint64_t>(), st.psummary.as<uint64_t>(),
                       st.stream);
}

// MEM: the first pass (offset 0 of every read), then the plan
template <typename IDX>
int mem_plan(QueryRun &st, const DevIndex<IDX> &ix)
{
  const vsa_index *index = st.index;
  const uint64_t nq = st.queries->nq;
  // one bit per text position: does its suffix have a neighbour in the
  // suffix array with lcp >= L?  Made once per (index, L), kept.
  if (index->repbits == nullptr || index->repleast != st.searchlength)
  {
    if (index->repbits == nullptr)
    {
      VSA_HIP(vsa_hip_malloc((void **) &index->repbits,
                             ((index->n + 1) / 32 + 4) * 4));
    }
    VSA_HIP(hipMemsetAsync(index->repbits, 0, ((index->n + 1) / 32 + 4) * 4,
                           st.stream));
    k_repeat_bits<IDX><<<vsa_grid(blocksfor((index->n + 16) / 16)),
                         VSA_BLOCK, 0, st.stream>>>(
        ix.lcp, ix.suf, index->n, st.searchlength, index->repbits);
    VSA_HIP(hipGetLastError());
    index->repleast = st.searchlength;
  }
  const Form first = pickform(index, st.queries, st.qs, Stage::MemFirst,
                              st.searchlength);
  PlanEmit em;
  // (a read answers at most one offset per round)
  if (alloc_first(st) || first_pass(st, ix, first, nullptr) ||
      plan_emit(st, VSA_PLAN_ROUNDS, &em))
  {
    return -100;
  }
  k_mem_plan<IDX><<<gridfor(nq), VSA_BLOCK, 0, st.stream>>>(
      ix, st.qs, st.perquery, st.searchlength, st.wfirste.as<uint32_t>(),
      st.wfmdb.as<uint64_t>(), index->repbits, st.wcount.as<uint32_t>(),
      st.wplan.as<PlanRanges>(), em);
  VSA_HIP(hipGetLastError());
  VSA_HIP(plan_summary(st));
  st.fromplan = true;
  st.plansearches = nq; // (an upper bound of the plan's own locates per round)
  return 0;
}

// VSA_DEBUG_PLANFILE: the plans of the first 65 536 queries as they stand
// when the search kernel starts -- per query its count and VSA_PLAN_RANGES
// ranges (first | length << 16), 32-bit words -- for bench.py, which prices
// the kernel on exactly the searches it runs
int dump_planfile(QueryRun &st, const char *pf)
{
  const uint64_t k = std::min<uint64_t>(st.queries->nq, 65536);
  std::vector<uint32_t> hc(k), hp(k * VSA_PLAN_RANGES);
  VSA_HIP(hipMemcpyAsync(hc.data(), st.wcount.p, k * 4,
                         hipMemcpyDeviceToHost, st.stream));
  VSA_HIP(hipMemcpyAsync(hp.data(), st.wplan.p, k * sizeof(PlanRanges),
                         hipMemcpyDeviceToHost, st.stream));
  VSA_HIP(hipStreamSynchronize(st.stream));
  if (FILE *f = fopen(pf, "wb"))
  {
    for (uint64_t q = 0; q < k; q++)
    {
      (void) fwrite(&hc[q], 4, 1, f);
      (void) fwrite(&hp[q * VSA_PLAN_RANGES], 4, VSA_PLAN_RANGES, f);
    }
    fclose(f);
  }
  return 0;
}

// MUM: the first pass, the reads it has not finished as a list, their plans
template <typename IDX>
int mum_plan(QueryRun &st, const DevIndex<IDX> &ix)
{
  const uint64_t nq = st.queries->nq;
  if (alloc_first(st) || st.wlist.alloc(nq * 4))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(st.wcount.as<uint32_t>() + nq, 0, 4, st.stream));
  // per workgroup of the first pass: reads it leaves to the plan | reads
  // whose offset 0 is a candidate (counted by the first pass itself)
  const uint64_t nb = blocksfor(nq), nbr = vsa_grid_blocks(nb);
  DevBuf bcount;
  if (bcount.alloc((nbr + 1) * 8) || st.wboffset.alloc((nbr + 1) * 8))
  {
    return -100;
  }
  // (both halves of a count stay below 2^32: nq does)
  VSA_HIP(hipMemsetAsync(bcount.as<uint64_t>() + nb, 0, 8, st.stream));
  if (first_pass(st, ix, st.form, bcount.as<uint64_t>()))
  {
    return -100;
  }
  // the reads the first pass has not finished, as a list (its counts per
  // workgroup, a scan over the workgroups, an ordered fill); with it come
  // the places of the first pass's candidates
  VSA_HIP(rocprim_run(st.wtemp, [&](void *p, size_t &tb) {
    return rocprim::exclusive_scan(p, tb, bcount.as<uint64_t>(),
                                   st.wboffset.as<uint64_t>(), (uint64_t) 0,
                                   (size_t) (nb + 1), rocprim::plus<uint64_t>(),
                                   st.stream);
  }));
  k_wanted_fill<<<vsa_grid(nb), VSA_BLOCK, 0, st.stream>>>(
      st.wcount.as<uint32_t>(), nq, 0u, st.wboffset.as<uint64_t>(),
      st.wlist.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  // (the length of the list and the number of first-pass candidates,
  // wboffset[nb], come to the host with the counts behind the search
  // kernel: no wait here -- the plan kernel is launched over all reads
  // and reads the length on the device)
  st.nlistword = st.wboffset.as<uint64_t>() + nb;
  // on the deep tables the plan answers the offsets it locates itself (room
  // for every search A of a list of all reads: its length is not known here)
  PlanEmit em = PlanEmit();
  if (st.form != Form::Ref && plan_emit(st, VSA_PLAN_ROUNDS - 1, &em))
  {
    return -100;
  }
  withform(st.form, [&](auto deep, auto, auto rows, auto) {
    k_mum_plan<IDX, deep, deep, rows><<<gridfor(nq), VSA_BLOCK, 0, st.stream>>>(
        ix, st.qs, st.wlist.as<uint32_t>(), st.nlistword, st.searchlength,
        st.wfirste.as<uint32_t>(), st.wcount.as<uint32_t>(),
        st.wplan.as<PlanRanges>(), em);
  });
  if (st.planemit)
  {
    VSA_HIP(plan_summary(st));
  }
  VSA_HIP(hipGetLastError());
  const char *pf = getenv("VSA_DEBUG_PLANFILE");
  if (pf != nullptr && dump_planfile(st, pf))
  {
    return -100;
  }
  st.fromplan = true;
  return 0;
}

// does the planned MUM search take its chunks from the tile queue
// (k_mum_walk_tiles)?  VSA_TUNE=32: the workgroup tiles of
// k_query_search_planned, which the MEM plan goes through anyway
bool tilequeue(const QueryRun &st)
{
  return st.fromplan && st.domum && (st.index->tune & 32u) == 0;
}

// workgroups of the tile queue: VSA_WALK_GRID, or what the device holds at
// once (the kernel's occupancy times the compute units; kept in the index)
template <typename IDX>
int walkgrid(const QueryRun &st, uint32_t *grid)
{
  const vsa_index *index = st.index;
  if (index->walkgridasked != 0)
  {
    *grid = index->walkgridasked;
    return 0;
  }
  hipError_t e = hipSuccess;
  withform(st.form, [&](auto deep, auto, auto rows, auto) {
    uint32_t &kept = index->walkgrid[deep ? 1 : 0][rows ? 1 : 0];
    if (kept == 0)
    {
      int percu = 0, cus = 0;
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
          &percu, k_mum_walk_tiles<IDX, deep, rows>, 256, 0);
      if (e == hipSuccess)
      {
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                                  index->device);
      }
      if (e == hipSuccess)
      {
        kept = (uint32_t) std::max(percu, 1) * (uint32_t) std::max(cus, 1);
      }
    }
    *grid = kept;
  });
  VSA_HIP(e);
  return 0;
}

// the search kernel: the planned form behind a plan (nplanblocks workgroups:
// of the tile queue, or one per perblock reads), else every (query, offset)
// pair (MEM, and MUM batches without a plan); regions: the cursor regions the
// tile queue spreads its workgroups over (a power of two)
template <typename IDX>
void launch_search(QueryRun &st, const DevIndex<IDX> &ix,
                   uint64_t nplanblocks, uint32_t regions)
{
  withform(st.form, [&](auto deep, auto, auto rows, auto) {
    auto tiles = [&]() {
      // (the tile counter: behind the cursors, zeroed with them)
      unsigned long long *cursors = st.cursor.as<unsigned long long>();
      k_mum_walk_tiles<IDX, deep, rows>
          <<<vsa_grid(nplanblocks), 256, 0, st.stream>>>(
              ix, st.qs, st.dbase, st.perquery, st.wplan.as<PlanRanges>(),
              st.wcount.as<uint32_t>(), st.wlist.as<uint32_t>(), st.nlistword,
              cursors + (size_t) VSA_CURSOR_SHARDS * VSA_CURSOR_STRIDE,
              st.searchlength, st.rawout.as<vsa_match>(),
              st.rawkeys.as<uint64_t>(), st.shardcap, regions - 1, cursors,
              st.rec.packbits, st.rec.valbits,
              st.blocksum.as<PlannedWork>(), st.index->walkshift);
    };
    auto planned = [&](auto mum) {
      k_query_search_planned<IDX, 256, deep, rows, mum>
          <<<vsa_grid(nplanblocks), 256, 0, st.stream>>>(
              ix, st.qs, st.dbase, st.perquery, st.wplan.as<PlanRanges>(),
              st.wcount.as<uint32_t>(), st.searchlength,
              st.rawout.as<vsa_match>(), st.rawkeys.as<uint64_t>(),
              st.shardcap, VSA_CURSOR_SHARDS - 1,
              st.cursor.as<unsigned long long>(), st.rec.packbits,
              st.rec.valbits, st.blocksum.as<PlannedWork>(),
              st.index->walkshift);
    };
    auto unplanned = [&](auto mum) {
      k_query_search<IDX, mum, deep, 256>
          <<<vsa_grid((st.nitems + 255) / 256), 256, 0, st.stream>>>(
              ix, st.qs, st.dbase, st.perquery, st.nitems, st.searchlength,
              st.rawout.as<vsa_match>(), st.rawkeys.as<uint64_t>(),
              st.shardcap, VSA_CURSOR_SHARDS - 1,
              st.cursor.as<unsigned long long>(), st.rec.packbits,
              st.rec.valbits);
    };
    if (tilequeue(st))
    {
      tiles();
    } else if (st.fromplan && st.domum)
    {
      planned(std::true_type());
    } else if (st.fromplan)
    {
      if constexpr (deep && !rows) // (the MEM plan: deep tables, bytes)
      {
        planned(std::false_type());
      }
    } else if (st.nitems > 0 && st.domum)
    {
      unplanned(std::true_type());
    } else if (st.nitems > 0)
    {
      unplanned(std::false_type());
    }
  });
}

// The search into cursor regions.  First guess of their size: MUM modes
// report at most one match per work-item but typically about one per query;
// MEM is unbounded.  The kernel counts what it needs and never writes past a
// region's capacity; on overflow of any region run again with regions of the
// size that was asked for.  (The tile queue: which wavefront takes which tile
// differs from launch to launch, and with it what a region receives.  Its
// second attempt writes everything into ONE region with room for all that
// was asked for, a number that does not depend on the schedule; the regions
// behind it stay empty and are never looked at.)
template <typename IDX>
int search(QueryRun &st, const DevIndex<IDX> &ix)
{
  const uint32_t nshards = VSA_CURSOR_SHARDS;
  // (reads per workgroup of k_query_search_planned<IDX, 256>)
  const uint64_t perblock = 256 * (st.domum ? VSA_WALK_READS : 1);
  uint64_t nplanblocks = (st.queries->nq + perblock - 1) / perblock;
  // entries of blocksum: one per workgroup, or (the tile queue) per wavefront
  uint64_t persum = 1;
  size_t rbytes = 0;
  if (tilequeue(st))
  {
    uint32_t grid = 0;
    if (walkgrid<IDX>(st, &grid))
    {
      return -100;
    }
    nplanblocks = grid;
    persum = 4;
  }
  const uint64_t nsums = persum * nplanblocks;
  if (st.fromplan)
  {
    // the work of the planned search (the locates it really makes -- the
    // walk leaves planned offsets out -- and the offsets planned): summed per
    // workgroup or wavefront by the kernel, reduced behind it into the fifth
    // and sixth word of the shard summary
    if (st.blocksum.alloc((persum * vsa_grid_blocks(nplanblocks) + 1) *
                          sizeof(PlannedWork)))
    {
      return -100;
    }
    VSA_HIP(rocprim::reduce(nullptr, rbytes, st.blocksum.as<PlannedWork>(),
                            (PlannedWork *) nullptr, PlannedWork{0, 0},
                            (size_t) nsums, PlannedWorkPlus(), st.stream));
    if (st.rtemp.alloc(rbytes))
    {
      return -100;
    }
  }
  // (one more line behind the cursors: the tile counter of k_mum_walk_tiles)
  const size_t cursorbytes = (size_t) (nshards + 1) * VSA_CURSOR_STRIDE * 8;
  if (st.cursor.alloc(cursorbytes) || st.doff.alloc(nshards * 8) ||
      st.summary.alloc(6 * 8))
  {
    return -100;
  }
  st.shardcap =
      std::max<uint64_t>((st.queries->nq * 2 / nshards) * 5 / 4 + 64, 256);
  uint64_t maxshard = 0;
  uint32_t regions = nshards;
  for (int attempt = 0; attempt < 2; attempt++)
  {
    if (st.rawout.alloc(regions * st.shardcap * st.rec.recsize) ||
        st.rawkeys.alloc(regions * st.shardcap * 8))
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(st.cursor.p, 0, cursorbytes, st.stream));
    st.tsearch.start();
    launch_search(st, ix, nplanblocks, regions);
    st.tsearch.stop();
    VSA_HIP(hipGetLastError());
    if (st.fromplan)
    {
      // (words 4 and 5 of the summary: 16-byte aligned)
      VSA_HIP(rocprim::reduce(
          st.rtemp.p, rbytes, st.blocksum.as<PlannedWork>(),
          reinterpret_cast<PlannedWork *>(st.summary.as<uint64_t>() + 4),
          PlannedWork{0, 0}, (size_t) nsums, PlannedWorkPlus(), st.stream));
    }
    // where each region goes in the dense list, how much there is
    const uint64_t *sm = st.summary.as<uint64_t>();
    VSA_HIP(shard_summary(st.cursor.as<unsigned long long>(), nshards,
                          st.doff.as<uint64_t>(), st.summary.as<uint64_t>(),
                          st.stream));
    const Fetch f[8] = {{sm, 8}, {sm + 1, 8}, {sm + 2, 8}, {sm + 3, 8},
                        {sm + 4, 8}, {st.planemit ? st.psummary.p : sm, 8},
                        {st.nlistword != nullptr ? st.nlistword : sm, 8},
                        {sm + 5, 8}};
    uint64_t got[8];
    if (fetchwords(st.stream, f, 8, got))
    {
      return -100;
    }
    if (st.nlistword != nullptr)
    {
      st.nfirst = got[6] >> 32;
      st.plansearches = 2 * (got[6] & 0xFFFFFFFFull);
    }
    st.nplan = st.planemit ? got[5] : 0;
    st.needed = got[0];
    maxshard = got[1];
    st.plannedlocates = st.fromplan ? got[4] : 0;
    st.plannedwork = st.fromplan ? got[7] : 0;
    st.searchms += st.tsearch.ms();
    if (maxshard <= st.shardcap)
    {
      return 0;
    }
    st.shardcap = maxshard;
    if (tilequeue(st))
    {
      regions = 1;
      st.shardcap = st.needed;
    }
  }
  VSA_ERROR("match buffer overflow: %llu > %llu",
            (unsigned long long) maxshard, (unsigned long long) st.shardcap);
  return -5;
}

// the search's answers, the plan's and the first pass's into one dense list
int compact(QueryRun &st)
{
  const uint64_t total = st.needed + st.nplan + st.nfirst;
  if (total == 0)
  {
    return 0;
  }
  if (st.out.alloc(total * st.rec.recsize) || st.keys.alloc(total * 8) ||
      (st.nplan > 0 &&
       compact_into(st.rec, st.prawout, st.prawkeys, st.pcap, st.pcursor,
                    st.pdoff, st.out, st.keys, st.needed, st.stream)) ||
      (st.needed > 0 &&
       compact_into(st.rec, st.rawout, st.rawkeys, st.shardcap, st.cursor,
                    st.doff, st.out, st.keys, 0, st.stream)))
  {
    return -100;
  }
  if (st.nfirst > 0)
  {
    k_append_first<<<gridfor(st.queries->nq), VSA_BLOCK, 0, st.stream>>>(
        st.wfmlen.as<uint32_t>(), st.wfmdb.as<uint64_t>(),
        st.wboffset.as<uint64_t>(), st.queries->nq, st.perquery, st.dbase,
        st.qs.seqoffset, st.needed + st.nplan, st.out.as<vsa_match>(),
        st.keys.as<uint64_t>(), st.rec.packbits, st.rec.valbits);
    VSA_HIP(hipGetLastError());
  }
  st.needed = total;
  return 0;
}

// Lists shorter than this are sorted by rocPRIM unless VSA_TUNE says
// otherwise: a speed heuristic only.  On a 300 Mbp and on a 3 Gbp index (16-
// byte staging entries below 45 k candidates there) the bucket path won at
// every size tried, from 19 k candidates on (profiles/r05/sizes_probe.txt,
// sizes_probe_3g.txt); below the smallest size measured things stay as they
// were.
#define VSA_CS_MINPAIRS (1u << 14)

// bucket sorts run, calls that came back from one to rocPRIM (a bucket
// overflowed), calls that came back for the second attempt (a run was too
// long), and the geometry of the last one: for tests and probes
// (vsa_debug_candidate_sort; not part of the ABI)
std::atomic<uint64_t> g_cs_runs{0}, g_cs_overflows{0}, g_cs_longruns{0},
    g_cs_shift{0}, g_cs_buckets{0};

// -mum on packed records: does the sort read the candidates where they were
// produced (candidate_sort.inc), without compact()?
bool feedsbuckets(const QueryRun &st)
{
  const uint64_t total = st.needed + st.nplan + st.nfirst;
  const uint32_t tune = st.index->tune;
  // (beyond VSA_CS_MAXBUCKETS buckets, some 25 M candidates: a scatter
  // workgroup's counters no longer fit into LDS)
  if (!(st.domum && !st.domumcand && st.rec.packed && (tune & 4u) == 0 &&
        total > 0 && (total >= VSA_CS_MINPAIRS || (tune & 8u) != 0) &&
        cs_geometry(st.index->n, total, st.rec.lenbits, st.rec.dbbits)
                .nbuckets <= VSA_CS_MAXBUCKETS))
  {
    return false;
  }
  // (an index whose last batches overflowed the buckets: see cs_skip)
  if ((tune & 8u) == 0 && st.index->cs_skip > 0)
  {
    st.index->cs_skip--;
    return false;
  }
  return true;
}

// MUMs of a packed run through the buckets, sorted and filtered by runs
// there; c->flags != 0: the list has to go through compact() and rocPRIM
template <typename VAL>
int mumfilter_buckets(QueryRun &st, DevBuf &mums, MumCounts *c)
{
  const RecordForm &rec = st.rec;
  const uint64_t total = st.needed + st.nplan + st.nfirst;
  CsSources src = CsSources();
  if (st.needed > 0)
  {
    src.reg[0] = {st.rawout.p, st.rawkeys.as<uint64_t>(),
                  st.cursor.as<unsigned long long>(), st.shardcap, st.needed};
  }
  if (st.nplan > 0)
  {
    src.reg[1] = {st.prawout.p, st.prawkeys.as<uint64_t>(),
                  st.pcursor.as<unsigned long long>(), st.pcap, st.nplan};
  }
  if (st.nfirst > 0)
  {
    src.first = {st.wfmlen.as<uint32_t>(), st.wfmdb.as<uint64_t>(),
                 st.queries->nq, st.qs.seqoffset, rec.packbits, rec.valbits};
  }
  CsGeometry g;
  if (mums.alloc(total * sizeof(vsa_match)))
  {
    return -100;
  }
  const PairRecord<VAL> pr = {rec.lenbits, rec.valbits,
                              sizeof(VAL) == 4 ? st.qs.seqoffset : 0};
  uint64_t got[3];
  if (candidate_bucketfilter<VAL>(src, total, st.index->n, rec.lenbits,
                                  rec.dbbits, 0, pr, st.stream,
                                  mums.as<vsa_match>(), got, &g))
  {
    return -100;
  }
  g_cs_runs++;
  g_cs_shift = g.shift;
  g_cs_buckets = g.nbuckets;
  c->nmums = got[0];
  c->sumlength = got[1];
  c->flags = got[2];
  return 0;
}

// the dense list into the result: the pairs themselves, the MUMs behind the
// filter, the candidates as they lie, or the matches in reference order;
// *mumsum: the sum of the MUMs' lengths if the filter made it
// (-mum on packed records: the bucket sort in front of the filter takes the
// candidates from their producers; the dense list is made only if it gives up)
int finish(QueryRun &st, vsa_result *res, uint64_t *mumsum)
{
  const RecordForm &rec = st.rec;
  bool allbits = false; // the packed list at once through its second attempt
  if (feedsbuckets(st))
  {
    DevBuf mums;
    MumCounts c;
    if (rec.valbits != 0 ? mumfilter_buckets<uint32_t>(st, mums, &c)
                         : mumfilter_buckets<uint64_t>(st, mums, &c))
    {
      return -100;
    }
    if (c.flags == 0)
    {
      st.index->cs_penalty = 0;
      res->stats.candidates = st.needed + st.nplan + st.nfirst;
      res->count = c.nmums;
      res->matches = (vsa_match *) mums.release();
      *mumsum = c.sumlength;
      return 0;
    }
    if ((c.flags & VSA_CS_OVERFLOW) != 0)
    {
      g_cs_overflows++;
      st.index->cs_penalty =
          std::min(64u, std::max(1u, 2 * st.index->cs_penalty));
      st.index->cs_skip = st.index->cs_penalty;
    } else
    {
      g_cs_longruns++;
      allbits = true; // (the buckets were fine: a run was too long)
    }
  }
  if (compact(st))
  {
    return -100;
  }
  const uint64_t needed = st.needed;
  res->stats.candidates = st.domum ? needed : 0;
  if (rec.keeppairs)
  {
    res->count = needed;
    res->packbits = rec.lenbits;
    if (needed > 0)
    {
      res->matches = (vsa_match *) st.keys.release();
      res->packvals = (uint64_t *) st.out.release();
    }
  } else if (st.domum && !st.domumcand)
  {
    DevBuf mums;
    MumCounts c = MumCounts();
    int rc;
    if (rec.valbits != 0)
    {
      rc = mumfilter_packed(
          st.keys.as<const uint64_t>(), st.out.as<const uint32_t>(), needed,
          PairRecord<uint32_t>{rec.lenbits, rec.valbits, st.qs.seqoffset},
          rec.dbbits, 0, allbits, st.stream, mums, &c);
    } else if (rec.packed)
    {
      rc = mumfilter_packed(st.keys.as<const uint64_t>(),
                            st.out.as<const uint64_t>(), needed,
                            PairRecord<uint64_t>{rec.lenbits, 0, 0},
                            rec.dbbits, 0, allbits, st.stream, mums, &c);
    } else
    {
      rc = mumuniqueinquery(st.out, needed, st.stream, mums, &c.nmums,
                            &c.sumlength, 0, st.index->n,
                            st.queries->maxlength);
    }
    if (rc != 0)
    {
      return -100;
    }
    *mumsum = c.sumlength;
    res->count = c.nmums;
    res->matches = (vsa_match *) mums.release();
  } else if (needed > 0 && !st.ordered && st.domum)
  {
    // candidates for a filter that sorts them anyway (multi-GPU -mum): as
    // they lie
    res->count = needed;
    res->matches = (vsa_match *) st.out.release();
  } else if (needed > 0)
  {
    // reference order = work-item order; appends of one work-item are
    // contiguous and in order, the radix sort is stable
    DevBuf sk, sm;
    if (sk.alloc(needed * 8) || sm.alloc(needed * sizeof(vsa_match)) ||
        sortbykey(st.keys.as<uint64_t>(), sk.as<uint64_t>(),
                  st.out.as<vsa_match>(), sm.as<vsa_match>(), needed,
                  bitsfor(st.nitems), st.stream))
    {
      return -100;
    }
    res->count = needed;
    res->matches = (vsa_match *) sm.release();
  }
  return 0;
}

// -l L (MEM), -mum cand, -mum: the stages above in order
template <typename IDX>
int run_query(const vsa_index *index, const vsa_queries *queries, bool domum,
              bool domumcand, uint32_t searchlength, vsa_result *res,
              bool ordered = true, uint32_t forcebits = 0)
{
  vsa_dev_set_stream(index->stream);
  QueryRun st(index, queries, domum, domumcand, ordered, searchlength);
  const DevIndex<IDX> ix = index->view<IDX>();
  if (workitems<IDX>(st))
  {
    return -100;
  }
  res->stats.searches = st.nitems;
  if (st.nitems == 0)
  {
    return 0;
  }
  st.tall.start();
  if (const int rc = recordform(index, queries, domum, domumcand, ordered,
                                forcebits, &st.rec))
  {
    return rc;
  }
  if (decide(st) || (st.memplan && mem_plan(st, ix)) ||
      (st.reduce && mum_plan(st, ix)))
  {
    return -100;
  }
  if (const int rc = search(st, ix))
  {
    return rc;
  }
  uint64_t mumsum = ~0ull;
  if (finish(st, res, &mumsum))
  {
    return -100;
  }
  st.tall.stop();
  VSA_HIP(hipStreamSynchronize(st.stream));
  res->stats.count = res->count;
  res->stats.search_kernel_ms = st.searchms;
  res->stats.anchor_ms = 0; // (the anchor pass of round 1 is gone)
  res->stats.first_kernel_ms = st.tfirst.ms();
  // (searches: the offsets the plans hold, whatever the walk leaves out of
  // them; kernel_searches: the locates the search kernel really made)
  res->stats.kernel_searches = st.fromplan ? st.plannedlocates : st.nitems;
  if (st.fromplan)
  {
    res->stats.searches = st.plannedwork + queries->nq + st.plansearches;
  }
  res->stats.total_device_ms = st.tall.ms();
  if (mumsum != ~0ull)
  {
    res->stats.sumlength = mumsum; // the filter summed the lengths already
    return 0;
  }
  if (st.rec.keeppairs)
  {
    res->stats.sumlength = 0; // of candidates: nobody asks
    return 0;
  }
  return sumlengths(res->matches, res->count, st.stream,
                    &res->stats.sumlength);
}

// What the query entries share: the checks on their arguments (searchlength:
// nullptr for -complete), then limits() -- each entry's own checks on
// lengths -- and run(IDX(), res) on a fresh result for the index's offset
// width.  The result goes to *result when run returns 0, and is freed
// otherwise.
template <typename Limits, typename Run>
int query_entry(const char *name, const vsa_index *index,
                const vsa_queries *queries, const uint64_t *searchlength,
                vsa_result **result, Limits limits, Run run)
{
  if (index == nullptr || queries == nullptr || result == nullptr)
  {
    VSA_ERROR("%s: NULL argument", name);
    return -1;
  }
  *result = nullptr;
  if (queries->device != index->device)
  {
    VSA_ERROR("queries live on device %d, index on device %d",
              queries->device, index->device);
    return -1;
  }
  if (index->bck == nullptr)
  {
    VSA_ERROR("table bck is not loaded");
    return -3;
  }
  // Vmengine/fquery.c:440-446
  if (searchlength != nullptr && *searchlength < index->pl)
  {
    VSA_ERROR("searchlength=%lu must be >= %lu=prefixlen",
              (unsigned long) *searchlength, (unsigned long) index->pl);
    return -2;
  }
  if (const int rc = limits())
  {
    return rc;
  }
  if (vsa_set_device(index->device) != 0)
  {
    return -100;
  }
  vsa_result *res = newresult(index->device);
  const int rc =
      (index->isize == 4) ? run(uint32_t(), res) : run(uint64_t(), res);
  if (rc != 0)
  {
    vsa_result_free(res);
    return rc;
  }
  *result = res;
  return 0;
}

// the check of both vsa_findmumcandidates entries on the search length
// (with the prefix length's message)
int mumlimit(const vsa_index *index, uint64_t searchlength)
{
  if (searchlength > 0xFFFFFFF0ull)
  {
    VSA_ERROR("searchlength=%lu must be >= %lu=prefixlen",
              (unsigned long) searchlength, (unsigned long) index->pl);
    return -2;
  }
  return 0;
}

} // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------

extern "C" int vsa_findcompletematches(const vsa_index *index,
                                       const vsa_queries *queries,
                                       vsa_result **result)
{
  uint64_t qlimit = 0;
  bool shortquery = false;
  const int rc = query_entry(
      "vsa_findcompletematches", index, queries, nullptr, result,
      [&] {
        if (queries->maxlength > 0xFFFFFFF0ull)
        {
          VSA_ERROR("query length beyond 32 bits is not supported");
          return -3;
        }
        return 0;
      },
      [&](auto idx, vsa_result *res) {
        // Vmengine/exactcompl.c:179-185: the first query shorter than
        // prefixlength stops the run; queries before it are still matched
        qlimit = queries->nq;
        if (queries->minlength < index->pl)
        {
          for (uint64_t q = 0; q < queries->nq; q++)
          {
            if (queries->hlength[q] < index->pl)
            {
              qlimit = q;
              shortquery = true;
              break;
            }
          }
        }
        return run_complete<decltype(idx)>(index, queries, qlimit, res);
      });
  if (rc == 0 && shortquery)
  {
    VSA_ERROR("patternlength=%lu must be >= %lu=prefixlen",
              (unsigned long) queries->hlength[qlimit],
              (unsigned long) index->pl);
    return -2;
  }
  return rc;
}

extern "C" int vsa_findmumcandidates(const vsa_index *index,
                                     const vsa_queries *queries,
                                     uint64_t searchlength, int ordered,
                                     vsa_result **result)
{
  if (ordered)
  {
    return vsa_findquerymatches(index, queries, 1, 1, searchlength, result);
  }
  return query_entry(
      "vsa_findmumcandidates", index, queries, &searchlength, result,
      [&] { return mumlimit(index, searchlength); },
      [&](auto idx, vsa_result *res) {
        return run_query<decltype(idx)>(index, queries, true, true,
                                        (uint32_t) searchlength, res, false);
      });
}

extern "C" int vsa_findmumcandidates_packed(const vsa_index *index,
                                            const vsa_queries *queries,
                                            uint64_t searchlength,
                                            uint32_t lengthbits,
                                            vsa_result **result)
{
  return query_entry(
      "vsa_findmumcandidates_packed", index, queries, &searchlength, result,
      [&] {
        if (const int rc = mumlimit(index, searchlength))
        {
          return rc;
        }
        if (lengthbits == 0)
        {
          lengthbits = bitsfor(queries->maxlength);
        }
        if (lengthbits > 16)
        {
          VSA_ERROR("packed candidates: at most 16 length bits");
          return -2;
        }
        return 0;
      },
      [&](auto idx, vsa_result *res) {
        return run_query<decltype(idx)>(index, queries, true, true,
                                        (uint32_t) searchlength, res, false,
                                        lengthbits);
      });
}

extern "C" int vsa_findquerymatches(const vsa_index *index,
                                    const vsa_queries *queries,
                                    int domaximaluniquematch,
                                    int domaximaluniquematchcandidates,
                                    uint64_t searchlength,
                                    vsa_result **result)
{
  return query_entry(
      "vsa_findquerymatches", index, queries, &searchlength, result,
      [&] {
        if (searchlength > 0xFFFFFFFFull ||
            queries->maxlength > 0xFFFFFFF0ull)
        {
          VSA_ERROR("query or search length beyond 32 bits is not "
                    "supported");
          return -3;
        }
        return 0;
      },
      [&](auto idx, vsa_result *res) {
        return run_query<decltype(idx)>(
            index, queries, domaximaluniquematch != 0,
            domaximaluniquematchcandidates != 0, (uint32_t) searchlength,
            res);
      });
}

static int mumfilter_entry(void *device_candidates, uint64_t ncandidates,
                           int device, uint64_t carry, vsa_result **result)
{
  if (result == nullptr || (device_candidates == nullptr && ncandidates > 0))
  {
    VSA_ERROR("vsa_mumuniqueinquery: NULL argument");
    return -1;
  }
  *result = nullptr;
  if (vsa_set_device(device) != 0)
  {
    return -100;
  }
  vsa_result *res = newresult(device);
  hipStream_t stream = nullptr; // default stream: no index handle here
  vsa_dev_set_stream(stream);
  Timer tall(stream);
  DevBuf cand, mums;
  cand.p = device_candidates; // borrowed, released below
  uint64_t nm = 0, sum = 0;
  tall.start();
  const int rc = mumuniqueinquery(cand, ncandidates, stream, mums, &nm, &sum,
                                  carry);
  tall.stop();
  cand.release();
  if (rc != 0)
  {
    vsa_result_free(res);
    return rc;
  }
  (void) hipStreamSynchronize(stream);
  res->count = nm;
  res->matches = (vsa_match *) mums.release();
  res->stats.count = nm;
  res->stats.candidates = ncandidates;
  res->stats.total_device_ms = tall.ms();
  res->stats.sumlength = sum;
  *result = res;
  return 0;
}

extern "C" int vsa_mumuniqueinquery(void *device_candidates,
                                    uint64_t ncandidates, int device,
                                    vsa_result **result)
{
  return mumfilter_entry(device_candidates, ncandidates, device, 0, result);
}

extern "C" int vsa_mumuniqueinquery_range(void *device_candidates,
                                          uint64_t ncandidates, int device,
                                          uint64_t carry_dbright,
                                          vsa_result **result)
{
  return mumfilter_entry(device_candidates, ncandidates, device,
                         carry_dbright, result);
}

// word 0 / word 1 of row i of (key, value) pairs
// word 0 (key) or 1 (value) of row i of two lists of rows laid end to end
struct RowWord
{
  const uint64_t *rows, *more;
  uint64_t nrows; // in `rows`
  uint32_t word;
  __device__ uint64_t operator()(size_t i) const
  {
    return i < nrows ? rows[2 * i + word] : more[2 * (i - nrows) + word];
  }
};

// pairs -> records, in place order (vsa_result_fetch of a packed result)
__global__ void __launch_bounds__(VSA_BLOCK)
k_unpack_pairs(const uint64_t *__restrict__ key,
               const uint64_t *__restrict__ val, uint64_t n,
               uint32_t packbits, vsa_match *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint64_t k = key[t], v = val[t], mask = (1ull << packbits) - 1;
    vsa_match m;
    m.length = mask - (k & mask);
    m.dbstart = k >> packbits;
    m.queryseq = v >> 16;
    m.querystart = v & 0xFFFFu;
    out[t] = m;
  }
}

int vsa_unpack_result(const vsa_result *r, uint64_t count, vsa_match *device)
{
  k_unpack_pairs<<<gridfor(count), VSA_BLOCK>>>(
      reinterpret_cast<const uint64_t *>(r->matches), r->packvals, count,
      r->packbits, device);
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipDeviceSynchronize());
  return 0;
}

extern "C" int vsa_mumuniqueinquery_range_packed2(const void *device_rows,
                                                  uint64_t nrows,
                                                  const void *more_rows,
                                                  uint64_t nmore,
                                                  uint32_t lengthbits,
                                                  uint64_t totallength,
                                                  int device,
                                                  uint64_t carry_dbright,
                                                  vsa_result **result)
{
  if (result == nullptr || (device_rows == nullptr && nrows > 0) ||
      (more_rows == nullptr && nmore > 0) || lengthbits == 0 ||
      lengthbits > 16 || lengthbits + bitsfor(totallength) > 64)
  {
    VSA_ERROR("vsa_mumuniqueinquery_range_packed: bad argument");
    return -1;
  }
  *result = nullptr;
  if (vsa_set_device(device) != 0)
  {
    return -100;
  }
  vsa_result *res = newresult(device);
  hipStream_t stream = nullptr; // default stream: no index handle here
  vsa_dev_set_stream(stream);
  Timer tall(stream);
  DevBuf mums;
  MumCounts c = MumCounts();
  const uint64_t total = nrows + nmore;
  tall.start();
  int rc = 0;
  if (total > 0)
  {
    // the sort reads the rows as they lie (the first pass of the radix sort
    // takes iterators): no split into two arrays, no copy of the two lists
    // into one
    const uint64_t *rows = reinterpret_cast<const uint64_t *>(device_rows),
                   *more = reinterpret_cast<const uint64_t *>(more_rows);
    auto rowkeys = rocprim::make_transform_iterator(
        rocprim::counting_iterator<size_t>(0), RowWord{rows, more, nrows, 0});
    auto rowvals = rocprim::make_transform_iterator(
        rocprim::counting_iterator<size_t>(0), RowWord{rows, more, nrows, 1});
    rc = mumfilter_packed(rowkeys, rowvals, total,
                          PairRecord<uint64_t>{lengthbits, 0, 0},
                          bitsfor(totallength), carry_dbright, false, stream,
                          mums, &c);
  }
  tall.stop();
  if (rc != 0)
  {
    vsa_result_free(res);
    return rc;
  }
  (void) hipStreamSynchronize(stream);
  res->count = c.nmums;
  res->matches = (vsa_match *) mums.release();
  res->stats.count = c.nmums;
  res->stats.candidates = total;
  res->stats.sumlength = c.sumlength;
  res->stats.total_device_ms = tall.ms();
  *result = res;
  return 0;
}

extern "C" int vsa_mumuniqueinquery_range_packed(const void *device_rows,
                                                 uint64_t nrows,
                                                 uint32_t lengthbits,
                                                 uint64_t totallength,
                                                 int device,
                                                 uint64_t carry_dbright,
                                                 vsa_result **result)
{
  return vsa_mumuniqueinquery_range_packed2(device_rows, nrows, nullptr, 0,
                                            lengthbits, totallength, device,
                                            carry_dbright, result);
}

// For tests and probes, not part of the ABI: how often this process sorted
// MUM candidates by buckets, how often a bucket overflowed and the list went
// to rocPRIM after all, how often a run was too long for the first attempt,
// and shift and number of buckets of the last bucket sort.
extern "C" void vsa_debug_candidate_sort(uint64_t out[5])
{
  out[0] = g_cs_runs;
  out[1] = g_cs_overflows;
  out[2] = g_cs_longruns;
  out[3] = g_cs_shift;
  out[4] = g_cs_buckets;
}
