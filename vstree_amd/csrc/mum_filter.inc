// K4: MUM candidates -> MUMs (kurtz/cleanMUMcand.c:55-118) -- kernels;
// included by esa_search.hip (one translation unit: the kernels share the
// device functions of esa_device.hpp and the host pipelines of esa_search.hip
// launch them).
//
// One filter behind every sort.  A candidate is a key dbstart << lenbits |
// (2^lenbits - 1 - length) and a value that travels with it; the key carries
// all the rule looks at.  With the reference's running `dbright` = the largest
// right end in front of a candidate (carry = its value in front of the list),
// candidate i survives iff it is not covered (dbright < its right end) and no
// other candidate with its dbstart is at least as long.  The keys arrive
//   sorted by dbstart ALONE (one radix pass saved): the
//     reference's order inside a run of equal dbstarts is "longest first", and
//     of such a run only the longest can survive, and only if no other member
//     is as long (the others find dbright at or beyond their right end).  That
//     is decidable without the order: earlier members of a survivor's own run
//     are shorter than it, so they do not disturb the running maximum, and the
//     run itself is looked at as a run.  Runs are short (two reads starting at
//     the same position); a run longer than VSA_RUN_LIMIT raises bit 0 of
//     *overflow and the caller sorts on all bits instead;
//   or sorted on ALL bits (that second attempt; records, whose values are
//     their indices): the longer members of the run are in front and in the
//     running maximum already, and an equal one, if any, is the next key.
// Either way the filter is five launches over tiles: a tile of VSA_FT_TILE
// keys knows the maximum of its right ends without knowing anything else
// (pass A), one workgroup turns the tile maxima into the running maximum in
// front of each tile (S1), every tile then decides its candidates for good,
// counts the survivors and sums their lengths (pass B), one workgroup turns
// the counts into offsets (S2), and the survivors are written in order (pass
// C) -- from the pair, or gathered from the caller's 32-byte records, which
// are touched only there.  (Until round 3: rocPRIM max-scan, flags, rocPRIM
// sum-scan, writer, reduce -- 0.3 ms for 11.6 M candidates, each pass paying
// its launch and a look-back chain over thousands of workgroups.)
//
// The bucket path (candidate_sort.inc) does not come through these tiles
// since round 12: k_cs_filter applies the rule of k_mumf_flags<false> to a
// bucket where its sort left it in LDS -- the running maximum in front of a
// bucket is what the scatter found reaching into it -- and k_mumf_scan<0>
// turns its survivors per bucket into offsets as it does for tiles.  Whoever
// changes the rule changes it there as well; tests/test_gpu_bucket_filter.py
// and test_gpu_candidate_sort.py hold both to the oracle's list.
//
// At the end of the file: the three kernels of the wide form, for records
// whose dbstart and length do not fit into one key.

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

// workgroup-wide exclusive scan of one value per thread; total = sum / max of
// all.  OP: 0 sum, 1 max.  sh: VSA_BLOCK / 64 + 1 words of LDS.
template <int OP>
__device__ __forceinline__ uint64_t vsa_block_exscan(uint64_t v, uint64_t *sh,
                                                     uint64_t &total)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint64_t o = vsa_shfl64(incl, (int) (lane >= (uint32_t) d ? lane - d : lane));
    if (lane >= (uint32_t) d)
    {
      incl = OP == 0 ? incl + o : (o > incl ? o : incl);
    }
  }
  if (lane == 63)
  {
    sh[wave] = incl;
  }
  __syncthreads();
  uint64_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < VSA_BLOCK / 64; w++)
  {
    const uint64_t x = sh[w];
    if (w < wave)
    {
      before = OP == 0 ? before + x : (x > before ? x : before);
    }
    all = OP == 0 ? all + x : (x > all ? x : all);
  }
  __syncthreads();
  total = all;
  // exclusive: what the lanes in front of this one hold
  const uint64_t prev = vsa_shfl64(incl, (int) (lane > 0 ? lane - 1 : 0));
  uint64_t mine = lane > 0 ? prev : 0;
  mine = OP == 0 ? mine + before : (before > mine ? before : mine);
  return mine;
}

// pass A: the largest right end of every tile
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_tilemax(const uint64_t *__restrict__ key, uint64_t n,
               unsigned int lenbits, uint64_t *__restrict__ tilemax)
{
  if (vsa_bid() * VSA_FT_TILE >= n) // (a launch folded into two dimensions)
  {
    return;
  }
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  const KeyToRightEnd rightend = {lenbits};
  const uint64_t i0 = (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_FT_ITEMS;
  uint64_t m = 0;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    if (i0 + k < n)
    {
      const uint64_t e = rightend(key[i0 + k]);
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

// pass B: keep flags (the running maximum from the tile's carry and the keys
// in front inside the tile; SORTED: keys sorted on all bits, else on dbstart
// alone, see above), the number of survivors and the sum of their lengths per
// tile.  The SORTED form does not touch *overflow.
template <bool SORTED>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_flags(const uint64_t *__restrict__ key, uint64_t n,
             unsigned int lenbits, const uint64_t *__restrict__ tilecarry,
             uint8_t *__restrict__ keep, uint64_t *__restrict__ tilecount,
             uint64_t *__restrict__ tilelen,
             unsigned int *__restrict__ overflow)
{
  if (vsa_bid() * VSA_FT_TILE >= n) // (a launch folded into two dimensions)
  {
    return;
  }
  __shared__ uint64_t sh[VSA_BLOCK / 64 + 1];
  const KeyToRightEnd rightend = {lenbits};
  const uint64_t i0 = (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_FT_ITEMS;
  uint64_t kk[VSA_FT_ITEMS], e[VSA_FT_ITEMS], m = 0;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    kk[k] = i0 + k < n ? key[i0 + k] : 0;
    e[k] = i0 + k < n ? rightend(kk[k]) : 0;
    m = e[k] > m ? e[k] : m;
  }
  uint64_t total;
  uint64_t run = vsa_block_exscan<1>(m, sh, total);
  const uint64_t carry = tilecarry[vsa_bid()];
  run = carry > run ? carry : run;
  uint32_t kept = 0, bits = 0;
  uint64_t len = 0;
  const uint64_t lenmask = (1ull << lenbits) - 1;
#pragma unroll
  for (int k = 0; k < VSA_FT_ITEMS; k++)
  {
    const uint64_t i = i0 + k;
    bool ok = i < n && run < e[k];
    if (SORTED)
    {
      // (same dbstart and same length = same key)
      ok = ok && !(i + 1 < n && key[i + 1] == kk[k]);
    } else if (ok)
    {
      const uint64_t d = kk[k] >> lenbits;
      uint32_t steps = 0;
      for (uint64_t j = i; j > 0 && (key[j - 1] >> lenbits) == d; j--)
      {
        if (rightend(key[j - 1]) >= e[k] || ++steps > VSA_RUN_LIMIT)
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
      for (uint64_t j = i + 1; ok && j < n && (key[j] >> lenbits) == d; j++)
      {
        if (rightend(key[j]) >= e[k] || ++steps > VSA_RUN_LIMIT)
        {
          ok = false;
        }
      }
      if (steps > VSA_RUN_LIMIT)
      {
        atomicOr(overflow, 1u);
      }
    }
    if (i < n)
    {
      run = e[k] > run ? e[k] : run;
    }
    bits |= ok ? 1u << (8 * k) : 0u;
    kept += ok ? 1u : 0u;
    len += ok ? lenmask - (kk[k] & lenmask) : 0;
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

// What pass C makes of a survivor.  From its pair -- VAL = uint64_t: value =
// queryseq << 16 | querystart; uint32_t: value = query number in the batch <<
// valbits | querystart, queryseq = that number + seqoffset:
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

// ... or the caller's record whose index the value is
struct GatheredRecord
{
  using VAL = uint32_t;
  const vsa_match *cand;
  __device__ void operator()(uint64_t, uint64_t v, vsa_match *dst) const
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(cand + v);
    const uint4 lo = src[0], hi = src[1];
    reinterpret_cast<uint4 *>(dst)[0] = lo;
    reinterpret_cast<uint4 *>(dst)[1] = hi;
  }
};

// pass C: the survivors as records, in order.  A tile is walked in rows of
// VSA_BLOCK consecutive candidates, one per thread, so that the records of
// neighbouring lanes lie next to each other in the output (four consecutive
// candidates per thread wrote 32 bytes per lane 128 bytes apart: 188 us
// instead of 100 for the 11 M records of the headline batch)
template <typename WRITER>
__global__ void __launch_bounds__(VSA_BLOCK)
k_mumf_write(const uint64_t *__restrict__ key,
             const typename WRITER::VAL *__restrict__ value,
             const uint8_t *__restrict__ keep, uint64_t n,
             const uint64_t *__restrict__ tileoff, WRITER write,
             vsa_match *__restrict__ out)
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
      write(key[i], value[i], out + slot);
    }
  }
}

// ---- wide records: dbstart and length as two sort keys, the filter on the
// sorted records themselves (mumfilter_wide)

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

__global__ void __launch_bounds__(VSA_BLOCK)
k_mum_rightends(const vsa_match *__restrict__ cand, uint64_t n,
                uint64_t *__restrict__ rightend)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < n)
  {
    rightend[i] = cand[i].dbstart + cand[i].length - 1;
  }
}

// dbright[i] = max(0, rightend[0..i)) is what the reference's running
// variable holds when it looks at candidate i.  Candidate i survives iff it
// is not covered (dbright < rightend) and its successor does not end at the
// same position with the same start.
__global__ void __launch_bounds__(VSA_BLOCK)
k_mum_flags(const vsa_match *__restrict__ cand,
            const uint64_t *__restrict__ rightend,
            const uint64_t *__restrict__ dbright, uint64_t n,
            uint8_t *__restrict__ keep)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i >= n)
  {
    return;
  }
  bool k = dbright[i] < rightend[i];
  if (k && i + 1 < n)
  {
    // dbright[i+1] = rightend[i] here
    if (rightend[i + 1] == rightend[i] &&
        cand[i + 1].dbstart == cand[i].dbstart)
    {
      k = false;
    }
  }
  keep[i] = k ? 1 : 0;
}
