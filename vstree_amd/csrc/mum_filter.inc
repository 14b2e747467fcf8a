// K4: MUM candidates -> MUMs (kurtz/cleanMUMcand.c:55-118) -- kernels;
// included by esa_search.hip (one translation unit: the kernels share the
// device functions of esa_device.hpp and the host pipelines of esa_search.hip
// launch them).
//
// One filter behind every sort, and one statement of its rule.  With the
// reference's running `dbright` = the largest right end in front of a
// candidate (carry = its value in front of the list), candidate i survives
// iff it is not covered (dbright < its right end) and no other candidate with
// its dbstart is at least as long.  The candidates arrive
//   sorted by dbstart ALONE (packed keys; one radix pass saved): the
//     reference's order inside a run of equal dbstarts is "longest first", and
//     of such a run only the longest can survive, and only if no other member
//     is as long (the others find dbright at or beyond their right end).  That
//     is decidable without the order: earlier members of a survivor's own run
//     are shorter than it, so they do not disturb the running maximum, and the
//     run itself is looked at as a run -- vsa_mum_alone_in_run.  Runs are
//     short (two reads starting at the same position); a run longer than
//     VSA_RUN_LIMIT raises bit 0 of *overflow and the caller sorts on all bits
//     instead;
//   or sorted by dbstart and, inside a run, longest first (that second
//     attempt; records): the longer members of the run are in front and in
//     the running maximum already, and an equal one, if any, is the next
//     candidate -- vsa_mum_twin_follows.
// Either way the filter is five launches over tiles: a tile of VSA_FT_TILE
// candidates knows the maximum of its right ends without knowing anything
// else (pass A), one workgroup turns the tile maxima into the running maximum
// in front of each tile (S1), every tile then decides its candidates for
// good, counts the survivors and sums their lengths (pass B), one workgroup
// turns the counts into offsets (S2), and the survivors are written in order
// (pass C).  (Until round 3: rocPRIM max-scan, flags, rocPRIM sum-scan,
// writer, reduce -- 0.3 ms for 11.6 M candidates, each pass paying its launch
// and a look-back chain over thousands of workgroups.)
//
// The tiles read the candidates through a view, of which there are two:
//   PackedCands  a key dbstart << lenbits | (2^lenbits - 1 - length), which
//                carries all the rule looks at, and a value that travels with
//                it; a survivor is written from the pair (PairRecord) or
//                gathered from the caller's 32-byte records (GatheredRecord),
//                which are touched only there;
//   RecordCands  32-byte records in the sorted order themselves, for lists
//                whose dbstart and length do not fit into one key or that
//                have 2^32 members and more (mumfilter_wide sorts them with
//                the keys of k_mum_keys, at the end of this file).
//
// The bucket path (candidate_sort.inc) does not come through these tiles:
// k_cs_filter calls vsa_mum_alone_in_run on a bucket where its sort left it
// in LDS -- the running maximum in front of a bucket is what the scatter
// found reaching into it -- and k_mumf_scan<0> turns its survivors per bucket
// into offsets as it does for tiles.

// right end of a candidate from its sort key
struct KeyToRightEnd
{
  unsigned int lenbits;
  __host__ __device__ uint64_t operator()(uint64_t k) const
  {
    const uint64_t lenmask = (1ull << lenbits) - 1;
    return (k >> lenbits) + (lenmask - (k & lenmask)) - 1;
  }
};

#define VSA_RUN_LIMIT 64
#define VSA_FT_ITEMS 4
#define VSA_FT_TILE (VSA_BLOCK * VSA_FT_ITEMS)

// ---- the rule

// Candidates sorted by dbstart alone: is candidate i, of dbstart d and right
// end e, the one longest member of its run of equal dbstarts?  keyat(j) = the
// key of candidate j, of which this looks at j < n only.  Both walks end
// after VSA_RUN_LIMIT steps at the latest, whatever the keys are, and then
// raise bit 0 of *overflow (the answer is "no", and not to be used).
template <typename KEYAT, typename IDX>
__device__ __forceinline__ bool
vsa_mum_alone_in_run(KEYAT keyat, unsigned int lenbits, IDX i, IDX n,
                     uint64_t d, uint64_t e, unsigned int *overflow)
{
  const KeyToRightEnd rightend = {lenbits};
  bool ok = true;
  uint32_t steps = 0;
  for (IDX j = i; j > 0 && (keyat(j - 1) >> lenbits) == d; j--)
  {
    if (rightend(keyat(j - 1)) >= e || ++steps > VSA_RUN_LIMIT)
    {
      ok = false;
      break;
    }
  }
  if (steps > VSA_RUN_LIMIT)
  {
    atomicOr(overflow, 1u);
  }
  steps = 0;
  for (IDX j = i + 1; ok && j < n && (keyat(j) >> lenbits) == d; j++)
  {
    if (rightend(keyat(j)) >= e || ++steps > VSA_RUN_LIMIT)
    {
      ok = false;
    }
  }
  if (steps > VSA_RUN_LIMIT)
  {
    atomicOr(overflow, 1u);
  }
  return ok;
}

// Candidates sorted by dbstart and, inside a run, longest first: does the
// next candidate have the dbstart and the length of candidate i?
template <typename CANDS>
__device__ __forceinline__ bool
vsa_mum_twin_follows(const CANDS &cands, uint64_t i, uint64_t n)
{
  return i + 1 < n && cands.twin(i, i + 1);
}

// ---- the views

// What pass C makes of a survivor of packed keys.  From its pair -- VAL =
// uint64_t: value = queryseq << 16 | querystart; uint32_t: value = query
// number in the batch << valbits | querystart, queryseq = that number +
// seqoffset:
template <typename V>
struct PairRecord
{
  using VAL = V;
  unsigned int lenbits, valbits;
  uint64_t seqoffset;
  __device__ void operator()(uint64_t kkey, uint64_t v, vsa_match *dst) const
  {
    const uint64_t lenmask = (1ull << lenbits) - 1;
    vsa_match m;
    m.length = lenmask - (kkey & lenmask);
    m.dbstart = kkey >> lenbits;
    if (sizeof(VAL) == 4)
    {
      m.queryseq = (v >> valbits) + seqoffset;
      m.querystart = v & ((1ull << valbits) - 1);
    } else
    {
      m.queryseq = v >> 16;
      m.querystart = v & 0xFFFFu;
    }
    *dst = m;
  }
};

__device__ __forceinline__ void vsa_copy_record(const vsa_match *from,
                                                vsa_match *dst)
{
  const uint4 *src = reinterpret_cast<const uint4 *>(from);
  const uint4 lo = src[0], hi = src[1];
  reinterpret_cast<uint4 *>(dst)[0] = lo;
  reinterpret_cast<uint4 *>(dst)[1] = hi;
}

// ... or the caller's record whose index the value is
struct GatheredRecord
{
  using VAL = uint32_t;
  const vsa_match *cand;
  __device__ void operator()(uint64_t, uint64_t v, vsa_match *dst) const
  {
    vsa_copy_record(cand + v, dst);
  }
};

// (Rule: the part of a view that passes A and B read -- one instance of
// their kernels for all writers)
struct PackedKeys
{
  const uint64_t *__restrict__ key;
  unsigned int lenbits;
  __device__ uint64_t dbstart(uint64_t i) const { return key[i] >> lenbits; }
  __device__ uint64_t length(uint64_t i) const
  {
    const uint64_t lenmask = (1ull << lenbits) - 1;
    return lenmask - (key[i] & lenmask);
  }
  // (same dbstart and same length = same key)
  __device__ bool twin(uint64_t i, uint64_t j) const
  {
    return key[i] == key[j];
  }
};

template <typename WRITER>
struct PackedCands : PackedKeys
{
  using Rule = PackedKeys;
  const typename WRITER::VAL *__restrict__ value;
  WRITER rec;
  __device__ void write(uint64_t i, vsa_match *dst) const
  {
    rec(key[i], value[i], dst);
  }
};

struct RecordCands
{
  using Rule = RecordCands;
  const vsa_match *__restrict__ rec;
  __device__ uint64_t dbstart(uint64_t i) const { return rec[i].dbstart; }
  __device__ uint64_t length(uint64_t i) const { return rec[i].length; }
  __device__ bool twin(uint64_t i, uint64_t j) const
  {
    return rec[i].dbstart == rec[j].dbstart && rec[i].length == rec[j].length;
  }
  __device__ void write(uint64_t i, vsa_match *dst) const
  {
    vsa_copy_record(rec + i, dst);
  }
};

// ---- the tiles

// workgroup-wide exclusive scan of one value per thread; total = sum / max of
// all.  OP: 0 sum, 1 max.  sh: VSA_BLOCK / 64 words of LDS.
template <int OP>
__device__ __forceinline__ uint64_t vsa_block_exscan(uint64_t v, uint64_t *sh,
                                                     uint64_t &total)
{
  return vsa_block_exclusive_scan<OP, VSA_BLOCK>(v, sh, total);
}

// pass A: the largest right end of every tile
template <typename CANDS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_tilemax(CANDS cands, uint64_t n, uint64_t *__restrict__ tilemax)
{
  if (vsa_bid() * VSA_FT_TILE >= n) // (a launch folded into two dimensions)
  {
    return;
  }
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  const uint64_t i0 = (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_FT_ITEMS;
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    if (i0 + k < n)
    {
      const uint64_t e = cands.dbstart(i0 + k) + cands.length(i0 + k) - 1;
      m = e > m ? e : m;
    }
  }
  uint64_t total;
  (void) vsa_block_exscan<1>(m, sh, total);
  if (threadIdx.x == 0)
  {
    tilemax[vsa_bid()] = total;
  }
}

// S1 / S2: one workgroup, exclusive scan of `count` values with a start
// value; OP as above; out[count] = the total
#define VSA_FT_SCANITEMS 16
template <int OP>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_scan(const uint64_t *__restrict__ in, uint64_t count, uint64_t start,
            uint64_t *__restrict__ out,
            const uint64_t *__restrict__ in2 = nullptr,
            uint64_t *__restrict__ out2 = nullptr)
{
  // (a second workgroup, if launched, scans in2 -> out2 the same way)
  if (blockIdx.x == 1)
  {
    in = in2;
    out = out2;
  }
  // (a thread takes 16 consecutive values: three turns of the workgroup for
  // the 11 k tiles of the headline batch)
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  uint64_t run = start;
  for (uint64_t b = 0; b < count; b += VSA_BLOCK * VSA_FT_SCANITEMS)
  {
    const uint64_t i0 = b + (uint64_t) threadIdx.x * VSA_FT_SCANITEMS;
    uint64_t v[VSA_FT_SCANITEMS], mine = 0;
#pragma unroll
    for (int k = 0; k < VSA_FT_SCANITEMS; k++)
    {
      v[k] = i0 + k < count ? in[i0 + k] : 0;
      mine = OP == 0 ? mine + v[k] : (v[k] > mine ? v[k] : mine);
    }
    uint64_t total;
    uint64_t ex = vsa_block_exscan<OP>(mine, sh, total);
    ex = OP == 0 ? run + ex : (ex > run ? ex : run);
#pragma unroll
    for (int k = 0; k < VSA_FT_SCANITEMS; k++)
    {
      if (i0 + k < count)
      {
        out[i0 + k] = ex;
      }
      ex = OP == 0 ? ex + v[k] : (v[k] > ex ? v[k] : ex);
    }
    run = OP == 0 ? run + total : (total > run ? total : run);
  }
  if (threadIdx.x == 0)
  {
    out[count] = run;
  }
}

// pass B: keep flags (the running maximum from the tile's carry and the
// candidates in front inside the tile; SORTED: longest first inside a run,
// else any order there and packed keys, see above), the number of survivors
// and the sum of their lengths per tile.  The SORTED form does not touch
// *overflow.
template <bool SORTED, typename CANDS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_flags(CANDS cands, uint64_t n, const uint64_t *__restrict__ tilecarry,
             uint8_t *__restrict__ keep, uint64_t *__restrict__ tilecount,
             uint64_t *__restrict__ tilelen,
             unsigned int *__restrict__ overflow)
{
  if (vsa_bid() * VSA_FT_TILE >= n) // (a launch folded into two dimensions)
  {
    return;
  }
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  const uint64_t i0 = (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_FT_ITEMS;
  uint64_t d[VSA_FT_ITEMS], l[VSA_FT_ITEMS], e[VSA_FT_ITEMS], m = 0;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    d[k] = i0 + k < n ? cands.dbstart(i0 + k) : 0;
    l[k] = i0 + k < n ? cands.length(i0 + k) : 0;
    e[k] = i0 + k < n ? d[k] + l[k] - 1 : 0;
    m = e[k] > m ? e[k] : m;
  }
  uint64_t total;
  uint64_t run = vsa_block_exscan<1>(m, sh, total);
  const uint64_t carry = tilecarry[vsa_bid()];
  run = carry > run ? carry : run;
  uint32_t kept = 0, bits = 0;
  uint64_t len = 0;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    const uint64_t i = i0 + k;
    bool ok = i < n && run < e[k];
    if constexpr (SORTED)
    {
      ok = ok && !vsa_mum_twin_follows(cands, i, n);
    } else if (ok)
    {
      ok = vsa_mum_alone_in_run(
          [&](uint64_t j) { return cands.key[j]; }, cands.lenbits, i, n, d[k],
          e[k], overflow);
    }
    if (i < n)
    {
      run = e[k] > run ? e[k] : run;
    }
    bits |= ok ? 1u << (8 * k) : 0u;
    kept += ok ? 1u : 0u;
    len += ok ? l[k] : 0;
  }
  // (n is padded to whole words of flags by the caller's allocation)
  *reinterpret_cast<uint32_t *>(keep + i0) = bits;
  uint64_t alltotal, alllen;
  (void) vsa_block_exscan<0>(kept, sh, alltotal);
  (void) vsa_block_exscan<0>(len, sh, alllen);
  if (threadIdx.x == 0)
  {
    tilecount[vsa_bid()] = alltotal;
    tilelen[vsa_bid()] = alllen;
  }
}

// pass C: the survivors as records, in order.  A tile is walked in rows of
// VSA_BLOCK consecutive candidates, one per thread, so that the records of
// neighbouring lanes lie next to each other in the output (four consecutive
// candidates per thread wrote 32 bytes per lane 128 bytes apart: 188 us
// instead of 100 for the 11 M records of the headline batch)
template <typename CANDS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_write(CANDS cands, const uint8_t *__restrict__ keep, uint64_t n,
             const uint64_t *__restrict__ tileoff, vsa_match *__restrict__ out)
{
  if (vsa_bid() * VSA_FT_TILE >= n) // (a launch folded into two dimensions)
  {
    return;
  }
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  uint64_t base = tileoff[vsa_bid()];
#pragma unroll
  for (int r = 0; r < VSA_FT_ITEMS; r++)
  {
    const uint64_t i = vsa_bid() * VSA_FT_TILE + (uint64_t) r * VSA_BLOCK +
                       threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    uint64_t total;
    const uint64_t slot = base + vsa_block_exscan<0>(k ? 1u : 0u, sh, total);
    base += total;
    if (k)
    {
      cands.write(i, out + slot);
    }
  }
}

// ---- wide records: dbstart and length as the keys of two stable sorts
// (mumfilter_wide); the sorted records then go through the tiles as
// RecordCands

__global__ void __launch_bounds__(VSA_BLOCK)
k_mum_keys(const vsa_match *__restrict__ cand, uint64_t n,
           uint64_t *__restrict__ keylen, uint64_t *__restrict__ keydb)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < n)
  {
    keylen[i] = ~cand[i].length; // decreasing length
    keydb[i] = cand[i].dbstart;
  }
}
