// Supermaximal repeats on the index, vmatch -supermax -l L IDX; included by
// esa_search.hip inside its anonymous namespace.
//
// Reference: findsupermax (Vmengine/fsuper.c:142-165) walks the lcp-interval
// tree (include/vdfstrav.c:247-420) and reports a node [left, right] of depth
// d when all its children are leaves ("alwaysontop", fsuper.c:11-19), d >= L
// and the characters to the left of its suffixes are pairwise different
// (special symbols not counted, the suffix at text position 0 once:
// verifysupermaximality, fsuper.c:60-103); every pair of suffixes of such a
// node is a match (selectsupermaxialrepeats, fsuper.c:105-127), delivered
// with the smaller start first (ACCEPTMATCH, Vmengine/fself.c:21-38).
//
// In lcp terms a node whose children are all leaves is a run: lcp[left] < d,
// lcp[left+1 .. right] == d, lcp[right+1] < d.  Runs start where the lcp
// value rises, which the bytes of lcptab decide (a byte of 255 is looked up
// in llv afterwards):
//   S1  select      suffix array positions c with lcp[c+1] >= L and
//                   lcp[c] < lcp[c+1] (or either byte 255): run candidates,
//                   in suffix array order = the reference's node order
//   S2  k_supermax_count   one work-item per candidate: exact depth, extent,
//                   left characters; number of pairs
//   S3  k_supermax_write   the pairs, s ascending, then t ascending


// ---- ordered selection of suffix array positions by their lcp bytes --------
//
// rocprim::select over a counting iterator with a predicate that reads two
// bytes per position runs at 86 G positions/s (35 ms for a 3 Gbp index); the
// two passes below read the lcp bytes sixteen at a time (count per workgroup,
// scan of the workgroup totals, write) and keep the positions in order.
//   SUPERMAX = false: positions i with lcp[i+1] >= lmin          (repeats)
//   SUPERMAX = true : ... and lcp[i] < lcp[i+1], or a byte of 255 (runs)
#define VSA_SEL_PER 16 // positions per work-item

template <bool SUPERMAX>
__device__ __forceinline__ uint32_t lcpsel_mask(const uint8_t *lcp,
                                                uint64_t n, uint64_t first,
                                                uint32_t lmin)
{
  // bytes lcp[first .. first+16]: lcp has n+1 entries and 32 bytes of slack
  uint32_t mask = 0;
  if (first >= n)
  {
    return 0;
  }
  const vsa_u128 v = vsa_load16(lcp + first);
  const uint8_t last = lcp[first + 16];
  uint8_t b[17];
  __builtin_memcpy(b, &v, 16);
  b[16] = last;
#pragma unroll
  for (int k = 0; k < VSA_SEL_PER; k++)
  {
    const uint32_t b1 = b[k + 1];
    bool ok = b1 >= lmin && b1 != 0 && first + k < n;
    if (SUPERMAX)
    {
      ok = ok && (first + k == 0 || b[k] < b1 || b1 == 255);
    }
    mask |= ok ? (1u << k) : 0u;
  }
  return mask;
}

template <bool SUPERMAX>
__global__ void __launch_bounds__(VSA_BLOCK)
k_lcpsel_count(const uint8_t *__restrict__ lcp, uint64_t n, uint32_t lmin,
               uint32_t *__restrict__ blocktotal)
{
  __shared__ uint32_t wavesum[VSA_BLOCK / 64];
  if (vsa_bid() * VSA_BLOCK * VSA_SEL_PER >= n) // (a folded launch's surplus)
  {
    return;
  }
  const uint64_t first =
      (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_SEL_PER;
  uint32_t c = (uint32_t) __builtin_popcount(
      lcpsel_mask<SUPERMAX>(lcp, n, first, lmin));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1)
  {
    c += __shfl_xor(c, d, 64);
  }
  if ((threadIdx.x & 63) == 0)
  {
    wavesum[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < VSA_BLOCK / 64; w++)
    {
      t += wavesum[w];
    }
    blocktotal[vsa_bid()] = t;
  }
}

// POS: the width of a suffix array position (uint32_t, or uint64_t for texts of
// 2^32 symbols and more)
template <bool SUPERMAX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_lcpsel_write(const uint8_t *__restrict__ lcp, uint64_t n, uint32_t lmin,
               const uint64_t *__restrict__ blockoffset,
               POS *__restrict__ out)
{
  __shared__ uint32_t wavesum[VSA_BLOCK / 64];
  if (vsa_bid() * VSA_BLOCK * VSA_SEL_PER >= n) // (a folded launch's surplus)
  {
    return;
  }
  const uint64_t first =
      (vsa_bid() * VSA_BLOCK + threadIdx.x) * VSA_SEL_PER;
  uint32_t mask = lcpsel_mask<SUPERMAX>(lcp, n, first, lmin);
  uint32_t total;
  uint64_t slot = blockoffset[vsa_bid()] +
                  vsa_block_exclusive_scan<0, VSA_BLOCK>(
                      (uint32_t) __builtin_popcount(mask), wavesum, total);
  while (mask != 0)
  {
    const uint32_t k = (uint32_t) __builtin_ctz(mask);
    mask &= mask - 1;
    out[slot++] = (POS) (first + k);
  }
}

// out (device, room for n entries) = the selected positions in ascending
// order; *count = how many
template <bool SUPERMAX, typename POS>
static int lcp_select(const uint8_t *lcp, uint64_t n, uint32_t lmin,
                      hipStream_t stream, DevBuf &out, uint64_t *count)
{
  const uint64_t perblock = (uint64_t) VSA_BLOCK * VSA_SEL_PER;
  const uint64_t nblocks = (n + perblock - 1) / perblock;
  DevBuf totals, offsets, temp;

  *count = 0;
  if (n == 0)
  {
    return 0;
  }
  if (totals.alloc((nblocks + 1) * 4) || offsets.alloc((nblocks + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(hipMemsetAsync(totals.as<uint32_t>() + nblocks, 0, 4, stream));
  k_lcpsel_count<SUPERMAX><<<vsa_grid(nblocks), VSA_BLOCK, 0, stream>>>(
      lcp, n, lmin, totals.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  auto widen =
      rocprim::make_transform_iterator(totals.as<uint32_t>(), U32ToU64());
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::exclusive_scan(p, tb, widen, offsets.as<uint64_t>(),
                                   (uint64_t) 0, (size_t) (nblocks + 1),
                                   rocprim::plus<uint64_t>(), stream);
  }));
  const Fetch f = {offsets.as<uint64_t>() + nblocks, 8};
  if (fetchwords(stream, &f, 1, count))
  {
    return -100;
  }
  if (*count == 0)
  {
    return 0;
  }
  if (out.alloc(*count * sizeof(POS)))
  {
    return -100;
  }
  k_lcpsel_write<SUPERMAX, POS><<<vsa_grid(nblocks), VSA_BLOCK, 0, stream>>>(
      lcp, n, lmin, offsets.as<uint64_t>(), out.as<POS>());
  VSA_HIP(hipGetLastError());
  return 0;
}

// lcp values along a walk that starts next to position p.  Values of 255 and
// more live in llv, sorted by index: one binary search finds where p stands
// among them, and the exceptions a walk meets on its way left (positions p-1,
// p-2, ...) or right (p+1, p+2, ...) are the neighbouring entries, in order
// (what the reference's getexception cache does, kurtz-basic/accvirt.c:69-150;
// a binary search per step cost the tandem kernel 80 % of its time).  Only a
// walk that compares with a depth of 255 or more needs the values at all: below
// that a byte of 255 is simply "larger".
template <typename IDX>
struct LcpCursor
{
  uint64_t left, right; // next exception to the left of / right of p
  __device__ __forceinline__ uint64_t start(const DevIndex<IDX> &ix,
                                            uint64_t p)
  {
    // returns lcp(p); call only if the byte of p is 255
    uint64_t lo = 0, hi = ix.nllv;
    while (lo < hi)
    {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if ((uint64_t) ix.llv[2 * mid] < p)
      {
        lo = mid + 1;
      } else
      {
        hi = mid;
      }
    }
    left = lo;      // exceptions with an index below p: 0 .. lo-1
    right = lo + 1; // the entry of p itself is lo
    return (uint64_t) ix.llv[2 * lo + 1];
  }
  // position x = the one left of the last one asked for (first: p - 1)
  __device__ __forceinline__ uint64_t goleft(const DevIndex<IDX> &ix,
                                             uint64_t x)
  {
    const uint64_t v = ix.lcp[x];
    return v < 255 ? v : (uint64_t) ix.llv[2 * (--left) + 1];
  }
  // position x = the one right of the last one asked for (first: p + 1)
  __device__ __forceinline__ uint64_t goright(const DevIndex<IDX> &ix,
                                              uint64_t x)
  {
    const uint64_t v = ix.lcp[x];
    return v < 255 ? v : (uint64_t) ix.llv[2 * (right++) + 1];
  }
};

template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_supermax_count(const DevIndex<IDX> ix, const POS *__restrict__ cand,
                 uint64_t ncand, uint64_t searchlength,
                 POS *__restrict__ right, uint64_t *__restrict__ depth,
                 uint64_t *__restrict__ counts)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= ncand)
  {
    return;
  }
  const uint64_t c = cand[t];
  // depth of the interval that starts at c; deep ones (255 and more) read
  // their neighbours' values through the cursor, the others from the bytes
  LcpCursor<IDX> cur;
  const bool big = ix.lcp[c + 1] == 255;
  const uint64_t d = big ? cur.start(ix, c + 1) : (uint64_t) ix.lcp[c + 1];
  uint64_t pairs = 0, r = c + 1;
  if (d >= searchlength &&
      (c == 0 || (big ? cur.goleft(ix, c) : (uint64_t) ix.lcp[c]) < d))
  {
    uint64_t next = 0; // lcp(r + 1), 0 behind the last suffix
    while (r + 1 <= ix.n)
    {
      next = big ? cur.goright(ix, r + 1) : (uint64_t) ix.lcp[r + 1];
      if (next != d)
      {
        break;
      }
      r++;
      next = 0;
    }
    if (!(r + 1 <= ix.n && next > d))
    {
      // verifysupermaximality: left characters pairwise different
      uint64_t seen[4] = {0, 0, 0, 0}; // one bit per symbol 0..255
      bool ok = true;
      for (uint64_t q = c; q <= r && ok; q++)
      {
        // the suffix at text position 0 carries 253 in bwt (chardef.h:31)
        const uint8_t cc = ix.bwt[q];
        if (!VSA_ISSPECIAL(cc))
        {
          const uint64_t bit = 1ull << (cc & 63);
          ok = (seen[cc >> 6] & bit) == 0;
          seen[cc >> 6] |= bit;
        }
      }
      if (ok)
      {
        const uint64_t k = r - c + 1;
        pairs = k * (k - 1) / 2;
      }
    }
  }
  right[t] = (POS) r;
  depth[t] = d;
  counts[t] = pairs;
}

template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_supermax_write(const DevIndex<IDX> ix, const POS *__restrict__ cand,
                 uint64_t ncand, const POS *__restrict__ right,
                 const uint64_t *__restrict__ depth,
                 const uint64_t *__restrict__ counts,
                 const uint64_t *__restrict__ offsets,
                 vsa_match *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= ncand || counts[t] == 0)
  {
    return;
  }
  const uint64_t c = cand[t], r = right[t];
  uint64_t slot = offsets[t];
  for (uint64_t s = c; s < r; s++)
  {
    const uint64_t i = (uint64_t) ix.suf[s];
    for (uint64_t u = s + 1; u <= r; u++)
    {
      const uint64_t j = (uint64_t) ix.suf[u];
      vsa_match m;
      m.length = depth[t];
      m.dbstart = i < j ? i : j;
      m.queryseq = i < j ? j : i;
      m.querystart = 0;
      out[slot++] = m;
    }
  }
}

template <typename IDX, typename POS>
int run_supermax(const vsa_index *index, uint64_t searchlength,
                 vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  const uint64_t n = index->n;
  DevBuf cand, right, depth, counts, offsets, matches;
  uint64_t ncand = 0, total = 0;

  res->stats.searches = n;
  tall.start();
  tsearch.start();
  if (lcp_select<true, POS>(ix.lcp, n,
                       (uint32_t) (searchlength < 255 ? searchlength : 255),
                       stream, cand, &ncand))
  {
    return -100;
  }
  tsearch.stop();
  res->stats.candidates = ncand;
  if (ncand > 0)
  {
    if (right.alloc(ncand * sizeof(POS)) || depth.alloc(ncand * 8) ||
        counts.alloc((ncand + 1) * 8) || offsets.alloc((ncand + 1) * 8))
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(counts.as<uint64_t>() + ncand, 0, 8, stream));
    k_supermax_count<IDX, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
        ix, cand.as<POS>(), ncand, searchlength, right.as<POS>(),
        depth.as<uint64_t>(), counts.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    if (exclusive_sum(counts.as<uint64_t>(), offsets.as<uint64_t>(), ncand,
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
      k_supermax_write<IDX, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
          ix, cand.as<POS>(), ncand, right.as<POS>(),
          depth.as<uint64_t>(), counts.as<uint64_t>(),
          offsets.as<uint64_t>(), matches.as<vsa_match>());
      VSA_HIP(hipGetLastError());
    }
  }
  return finish(res, matches, total, tall, tsearch, stream);
}

// ---- maximal repeats, vmatch -l L IDX --------------------------------------
//
// Reference: vmatmaxoutgeneric (Vmengine/vmatfind.c:487-541) walks the
// lcp-interval tree bottom-up (include/vdfstrav.c:247-420); every node of
// depth >= L keeps the suffix start positions below it in one list per left
// character and one list for the rest (special symbols, start of the text);
// when a child -- a leaf or a finished subtree -- is attached to its father,
// every pair (position already at the father, position of the child) whose
// left characters differ or are not regular symbols is reported with the
// father's depth (processleafedge :330-400, processbranch :413-473), smaller
// start first (ACCEPTMATCH, Vmengine/fself.c:21-38).
//
// Here the attachments are the unit of work.  A child is attached to a father
// of depth d exactly at a suffix array position p with lcp[p] = d >= L:
//   A = [l, p-1]  what the father holds already: l = the nearest position to
//                 the left of p with lcp[l] < d
//   B = [p, e]    the child: e + 1 = the nearest position to the right of p
//                 with lcp <= d
// The reference performs the attachments in the order of (e, then deeper
// father first) and reports the pairs of one attachment by nested loops over
// left-character classes and list positions, which makes the slot of a pair a
// closed formula of class counts and ranks (repeat_slot).  So:
//   R1  select          positions p with lcp[p] >= L
//   R2  k_rep_extent    one work-item per attachment: l, e, d, class counts,
//                       number of pairs
//   R3  radix sort of the attachments by (e, -d); exclusive scan of the counts
//   R4  k_rep_write     one work-item per attachment: the pairs, each into
//                       its slot -- the reference's order without a sort of
//                       the matches
// Alphabets up to VSA_REP_MAXC regular symbols.

#define VSA_REP_MAXC 32

__global__ void __launch_bounds__(VSA_BLOCK)
k_iota32(uint32_t *__restrict__ out, uint64_t n)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    out[t] = (uint32_t) t;
  }
}

template <typename IDX>
__device__ __forceinline__ uint32_t rep_class(const DevIndex<IDX> &ix,
                                              uint64_t q, uint32_t nc)
{
  // the suffix at text position 0 carries 253 in bwt: not a regular symbol
  const uint32_t c = ix.bwt[q];
  return c < nc ? c : nc;
}

template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_rep_extent(const DevIndex<IDX> ix, uint32_t nc,
             const POS *__restrict__ cand, uint64_t ncand,
             uint64_t searchlength, POS *__restrict__ evl,
             POS *__restrict__ eve, uint32_t *__restrict__ evd,
             uint64_t *__restrict__ counts)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= ncand)
  {
    return;
  }
  const uint64_t p = (uint64_t) cand[t] + 1;
  LcpCursor<IDX> cur; // see there: values of 255 and more along the walks
  const bool big = ix.lcp[p] == 255;
  const uint64_t d = big ? cur.start(ix, p) : (uint64_t) ix.lcp[p];
  uint64_t l = p - 1, e = p, count = 0;
  if (d >= searchlength)
  {
    while ((big ? cur.goleft(ix, l) : (uint64_t) ix.lcp[l]) >= d)
    {
      l--; // lcp[0] = 0 < d
    }
    while (e + 1 <= ix.n &&
           (big ? cur.goright(ix, e + 1) : (uint64_t) ix.lcp[e + 1]) > d)
    {
      e++;
    }
    uint32_t fa[VSA_REP_MAXC + 1], sb[VSA_REP_MAXC + 1];
    for (uint32_t c = 0; c <= nc; c++)
    {
      fa[c] = sb[c] = 0;
    }
    for (uint64_t q = l; q < p; q++)
    {
      fa[rep_class(ix, q, nc)]++;
    }
    for (uint64_t q = p; q <= e; q++)
    {
      sb[rep_class(ix, q, nc)]++;
    }
    uint64_t sbreg = 0;
    for (uint32_t c = 0; c < nc; c++)
    {
      sbreg += sb[c];
    }
    for (uint32_t c = 0; c < nc; c++)
    {
      count += (uint64_t) fa[c] * (sbreg - sb[c] + sb[nc]);
    }
    count += (uint64_t) fa[nc] * (sbreg + sb[nc]);
  }
  evl[t] = (POS) l;
  eve[t] = (POS) e;
  // (a depth of 2^32 and more -- a repeat of four billion symbols -- is cut
  // here; texts below 2^33 symbols cannot hold one)
  evd[t] = (uint32_t) (d < 0xFFFFFFFFull ? d : 0xFFFFFFFFull);
  counts[t] = count;
}

// sort key "e ascending, then d descending" in as few bits as the batch needs
// (bits of n + bits of the largest depth: at most 64 by the caller's check)
template <typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_rep_keys(const POS *__restrict__ eve, const uint32_t *__restrict__ evd,
           uint64_t *__restrict__ keys, uint64_t n, unsigned int dbits)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint64_t e = eve[t], d = evd[t];
    keys[t] = (e << dbits) | (((1ull << dbits) - 1) - d);
  }
}

__global__ void __launch_bounds__(VSA_BLOCK)
k_rep_gathercounts(const uint64_t *__restrict__ counts,
                   const uint32_t *__restrict__ order, uint64_t n,
                   uint64_t *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    out[t] = counts[order[t]];
  }
  if (t == 0)
  {
    out[n] = 0;
  }
}

template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_rep_write(const DevIndex<IDX> ix, uint32_t nc,
            const POS *__restrict__ cand,
            const uint32_t *__restrict__ order, uint64_t nevents,
            const POS *__restrict__ evl,
            const POS *__restrict__ eve,
            const uint32_t *__restrict__ evd,
            const uint64_t *__restrict__ offsets,
            vsa_match *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= nevents)
  {
    return;
  }
  const uint32_t ev = order[t];
  const uint64_t base = offsets[t];
  if (offsets[t + 1] == base)
  {
    return;
  }
  const uint64_t p = (uint64_t) cand[ev] + 1, l = evl[ev], e = eve[ev];
  const uint64_t d = evd[ev];
  uint32_t fa[VSA_REP_MAXC + 1], sb[VSA_REP_MAXC + 1], csb[VSA_REP_MAXC + 2],
      ra[VSA_REP_MAXC + 1];
  uint64_t offf[VSA_REP_MAXC + 1];
  for (uint32_t c = 0; c <= nc; c++)
  {
    fa[c] = sb[c] = ra[c] = 0;
  }
  for (uint64_t q = l; q < p; q++)
  {
    fa[rep_class(ix, q, nc)]++;
  }
  for (uint64_t q = p; q <= e; q++)
  {
    sb[rep_class(ix, q, nc)]++;
  }
  csb[0] = 0;
  for (uint32_t c = 0; c < nc; c++)
  {
    csb[c + 1] = csb[c] + sb[c];
  }
  const uint64_t sbreg = csb[nc], su = sb[nc];
  uint64_t acc = 0;
  for (uint32_t c = 0; c < nc; c++)
  {
    offf[c] = acc;
    acc += (uint64_t) fa[c] * (sbreg - sb[c] + su);
  }
  const uint64_t totalreg = acc;
  // processbranch's loops (vmatfind.c:433-469) as slot arithmetic:
  //  father class cf regular:  for every son class cs != cf, the pairs
  //    (father element a, son element b) by a, then b; behind them the son's
  //    non-regular positions, each with every father element of class cf
  //  father positions with a non-regular left character, one by one:
  //    all regular son classes in turn, then the son's non-regular positions
  for (uint64_t x = l; x < p; x++)
  {
    const uint32_t cx = rep_class(ix, x, nc);
    const uint64_t rx = ra[cx]++;
    const uint64_t sx = (uint64_t) ix.suf[x];
    uint32_t rb[VSA_REP_MAXC + 1];
    for (uint32_t c = 0; c <= nc; c++)
    {
      rb[c] = 0;
    }
    for (uint64_t y = p; y <= e; y++)
    {
      const uint32_t cy = rep_class(ix, y, nc);
      const uint64_t ry = rb[cy]++;
      uint64_t slot;
      if (cx < nc)
      {
        if (cy < nc)
        {
          if (cy == cx)
          {
            continue; // same left character: not left maximal
          }
          const uint64_t before = csb[cy] - (cx < cy ? sb[cx] : 0);
          slot = offf[cx] + (uint64_t) fa[cx] * before + rx * sb[cy] + ry;
        } else
        {
          slot = offf[cx] + (uint64_t) fa[cx] * (sbreg - sb[cx]) +
                 ry * fa[cx] + rx;
        }
      } else
      {
        slot = totalreg + rx * (sbreg + su) +
               ((cy < nc) ? (uint64_t) csb[cy] + ry : sbreg + ry);
      }
      const uint64_t sy = (uint64_t) ix.suf[y];
      vsa_match m;
      m.length = d;
      m.dbstart = sx < sy ? sx : sy;
      m.queryseq = sx < sy ? sy : sx;
      m.querystart = 0;
      out[base + slot] = m;
    }
  }
}

// ACCEPTMATCH for an index that holds queries (fself.c:29-37): only pairs
// of a database position and a query position
__global__ void __launch_bounds__(VSA_BLOCK)
k_rep_dbquery(const vsa_match *__restrict__ m, uint64_t n,
              uint64_t querysepposition, uint8_t *__restrict__ keep)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    keep[t] = (m[t].dbstart < querysepposition &&
               m[t].queryseq > querysepposition)
                  ? 1
                  : 0;
  }
}

// The largest depth decides how many bits of a key (depth, position) the
// sort has to look at: *dbits for the depth, *endbit for the whole key.
static int keybits(const char *what, const char *item, uint64_t maxd,
                   uint64_t n, unsigned int *dbits, unsigned int *endbit)
{
  *dbits = bitsfor(maxd);
  *endbit = *dbits + bitsfor(n);
  if (*endbit > 64)
  {
    VSA_ERROR("%s: a %s of %llu symbols in a text of %llu: the sort key does "
              "not fit 64 bits", what, item, (unsigned long long) maxd,
              (unsigned long long) n);
    return -3;
  }
  return 0;
}

// Intervals report in the order of their keys: order2[] = order[] sorted
// (stably) by bits [0, endbit) of keys[]; offsets[t] = the first slot of
// interval order2[t], which reports counts[order2[t]] matches; *total = the
// number of slots.  (offsets has n + 1 entries.)
static int reportorder(uint64_t *keys, uint32_t *order, const uint64_t *counts,
                       uint64_t n, unsigned int endbit, uint32_t *order2,
                       uint64_t *offsets, hipStream_t stream, uint64_t *total)
{
  DevBuf keys2, sorted, temp;
  if (keys2.alloc(n * 8) || sorted.alloc((n + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::radix_sort_pairs(p, tb, keys, keys2.as<uint64_t>(), order,
                                     order2, (size_t) n, 0u, endbit, stream);
  }));
  k_rep_gathercounts<<<gridfor(n), VSA_BLOCK, 0, stream>>>(
      counts, order2, n, sorted.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  return exclusive_sum(sorted.as<uint64_t>(), offsets, n, stream, total);
}

template <typename IDX, typename POS>
int run_repeats(const vsa_index *index, uint64_t searchlength,
                vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  const uint64_t n = index->n;
  const uint32_t nc = index->numofchars;
  DevBuf cand, dcount, temp, evl, eve, evd, counts, keys, order, order2,
      offsets, matches, keep, kept;
  uint64_t ncand = 0, total = 0;

  res->stats.searches = n;
  if (dcount.alloc(8))
  {
    return -100;
  }
  tall.start();
  if (lcp_select<false, POS>(ix.lcp, n,
                        (uint32_t) (searchlength < 255 ? searchlength : 255),
                        stream, cand, &ncand))
  {
    return -100;
  }
  res->stats.candidates = ncand;
  if (ncand >= 0xFFFFFFFFull)
  {
    VSA_ERROR("maximal repeats: %llu positions with lcp >= %llu: more than "
              "2^32 attachments are not supported",
              (unsigned long long) ncand, (unsigned long long) searchlength);
    return -3;
  }
  if (ncand > 0)
  {
    if (evl.alloc(ncand * sizeof(POS)) || eve.alloc(ncand * sizeof(POS)) ||
        evd.alloc(ncand * 4) || counts.alloc(ncand * 8) ||
        keys.alloc(ncand * 8) || order.alloc(ncand * 4) ||
        order2.alloc(ncand * 4) || offsets.alloc((ncand + 1) * 8))
    {
      return -100;
    }
    tsearch.start();
    k_rep_extent<IDX, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
        ix, nc, cand.as<POS>(), ncand, searchlength, evl.as<POS>(),
        eve.as<POS>(), evd.as<uint32_t>(), counts.as<uint64_t>());
    tsearch.stop();
    VSA_HIP(hipGetLastError());
    k_iota32<<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(order.as<uint32_t>(),
                                                       ncand);
    VSA_HIP(hipGetLastError());
    uint32_t maxd = 0;
    VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
      return rocprim::reduce(p, tb, evd.as<uint32_t>(), dcount.as<uint32_t>(),
                             (uint32_t) 0, (size_t) ncand,
                             rocprim::maximum<uint32_t>(), stream);
    }));
    VSA_HIP(hipMemcpyAsync(&maxd, dcount.p, 4, hipMemcpyDeviceToHost,
                           stream));
    VSA_HIP(hipStreamSynchronize(stream));
    unsigned int dbits, endbit;
    if (keybits("maximal repeats", "repeat", maxd, n, &dbits, &endbit))
    {
      return -3;
    }
    k_rep_keys<POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
        eve.as<POS>(), evd.as<uint32_t>(), keys.as<uint64_t>(), ncand, dbits);
    VSA_HIP(hipGetLastError());
    if (reportorder(keys.as<uint64_t>(), order.as<uint32_t>(),
                    counts.as<uint64_t>(), ncand, endbit,
                    order2.as<uint32_t>(), offsets.as<uint64_t>(), stream,
                    &total))
    {
      return -100;
    }
    if (total > 0)
    {
      if (matches.alloc(total * sizeof(vsa_match)))
      {
        return -100;
      }
      k_rep_write<IDX, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
          ix, nc, cand.as<POS>(), order2.as<uint32_t>(), ncand,
          evl.as<POS>(), eve.as<POS>(), evd.as<uint32_t>(),
          offsets.as<uint64_t>(), matches.as<vsa_match>());
      VSA_HIP(hipGetLastError());
      if (index->hasindexedqueries)
      {
        uint64_t nk = 0;
        if (keep.alloc(total) || kept.alloc(total * sizeof(vsa_match)))
        {
          return -100;
        }
        k_rep_dbquery<<<gridfor(total), VSA_BLOCK, 0, stream>>>(
            matches.as<vsa_match>(), total, index->querysepposition,
            keep.as<uint8_t>());
        VSA_HIP(hipGetLastError());
        if (compact_matches(matches.as<vsa_match>(), keep.as<uint8_t>(),
                            total, kept.as<vsa_match>(),
                            dcount.as<uint64_t>(), stream))
        {
          return -100;
        }
        VSA_HIP(hipMemcpyAsync(&nk, dcount.p, 8, hipMemcpyDeviceToHost,
                               stream));
        VSA_HIP(hipStreamSynchronize(stream));
        total = nk;
        vsa_dev_free(matches.release());
        matches.p = kept.release();
      }
    }
  }
  return finish(res, matches, total, tall, tsearch, stream);
}

// ---- right branching tandem repeats, vmatch -tandem -l L IDX ---------------
//
// Reference: findtandems (Vmengine/ftandem.c:24-304) hands every lcp-interval
// [left, right] of depth d >= L to processcompletenode when the bottom-up
// traversal (include/vdfstrav.c:247-420) completes it.  Two suffixes: a
// tandem if one starts d symbols behind the other (CHECKPAIR :60-71).  More:
// one findmaxprefixlen over the interval finds a suffix that begins with the
// interval's string twice (:235-241); from that witness all of them are
// enumerated, leftwards first, then rightwards (tandemleftright :105-186).  A
// repeat at v is reported unless it can be shifted right by one symbol
// (SHOWTANDEM :44-58, PROCESSSUFFIX :73-88).
//
// Here the lcp-interval is the unit of work, named by its first position p
// with lcp[p] = d:
//   T1  select         positions p with lcp[p] >= L
//   T2  k_tan_extent   per position: is it the first of its interval?  left,
//                      right; the range [a, b] of suffixes that begin with
//                      the interval's string twice (two binary searches; a
//                      suffix s begins with it twice iff the suffix s + d
//                      lies in the interval, too: inverse suffix array), the
//                      reference's witness (its binary search
//                      replayed on indices: the comparisons it makes are
//                      decided by "left of a", "inside", "right of b"), the
//                      number of repeats reported
//   T3  radix sort of the intervals by (right, deeper first) = the order in
//       which the traversal completes them; exclusive scan of the counts
//   T4  k_tan_write    the repeats of an interval into its slots, in the
//                      reference's order

template <typename POS>
struct TandemUnit
{
  uint32_t d;
  POS a, b, w; // b < a: nothing; w = all ones: pair, its text position in a
};

// window = text[s + d .. s + 2d) against alpha = text[alpha .. alpha + d):
// <0 smaller, 0 equal, >0 larger; special symbols and the end of the text are
// larger than every symbol (the order of the suffix array)
template <typename IDX>
__device__ __forceinline__ int tan_compare(const DevIndex<IDX> &ix, uint64_t s,
                                           uint64_t alpha, uint64_t d)
{
  // eight symbols per step (the text has 0xFF, a special symbol, behind its
  // end, and alpha's d symbols are regular: they are an lcp).  Round 2: 215 ->
  // 168 ms for the 3 Gbp probe; 64 symbols per step took the kernel from 40
  // to 82 VGPRs and 193 ms (profiles/r02/tandem_3G.log).  What the kernel
  // spends its time on is the NUMBER of comparisons: every position of a
  // tandem array names a nested interval of its own, each with two binary
  // searches of O(d) comparisons.
  const uint8_t *x = ix.tis + s + d, *y = ix.tis + alpha;
  for (uint64_t k = 0; k < d; k += 8)
  {
    const uint64_t a = s + d + k < ix.n + 8 ? vsa_load8(x + k)
                                            : ~0ull,
                   b = vsa_load8(y + k);
    const uint64_t m = (a ^ b) | vsa_specialmask(a);
    if (m != 0)
    {
      const uint32_t j = (uint32_t) __builtin_ctzll(m) >> 3;
      if (k + j >= d)
      {
        return 0;
      }
      const uint8_t xa = (uint8_t) (a >> (8 * j)), yb = (uint8_t) (b >> (8 * j));
      if (VSA_ISSPECIAL(xa))
      {
        return 1;
      }
      return xa < yb ? -1 : 1;
    }
  }
  return 0;
}

// PROCESSSUFFIX / SHOWTANDEM: is the repeat of length d at v reported?
template <typename IDX>
__device__ __forceinline__ bool tan_reported(const DevIndex<IDX> &ix,
                                             uint64_t v, uint64_t d)
{
  if (v + 2 * d == ix.n)
  {
    return true;
  }
  const uint8_t c1 = ix.tis[v], c2 = ix.tis[v + 2 * d];
  return c1 != c2 || VSA_ISSPECIAL(c1) || VSA_ISSPECIAL(c2);
}

// isa[suf[i]] = i
template <typename IDX>
__global__ void __launch_bounds__(VSA_BLOCK)
k_inverse_suf(const IDX *__restrict__ suf, uint64_t count,
              uint32_t *__restrict__ isa)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < count)
  {
    isa[suf[i]] = (uint32_t) i;
  }
}

// The inverse suffix array of an index (n + 1 < 2^32), made once and kept with
// it (4 bytes per position).  Calls on one index come from one thread at a
// time (include/vstree_amd.h), so no lock.
template <typename IDX>
int tan_inverse(const vsa_index *index, const uint32_t **isa)
{
  if (index->isa32 == nullptr)
  {
    const uint64_t count = index->n + 1;
    uint32_t *p = nullptr;
    VSA_HIP(vsa_hip_malloc((void **) &p, count * 4 + 16));
    k_inverse_suf<IDX><<<gridfor(count), VSA_BLOCK, 0, index->stream>>>(
        (const IDX *) index->suf, count, p);
    VSA_HIP(hipGetLastError());
    index->isa32 = p;
  }
  *isa = index->isa32;
  return 0;
}

// window of the suffix at s (text[s + d .. s + 2d)) against the string of the
// interval [l, r] of depth d: the suffix at s + d lies in front of the
// interval, inside it or behind it -- the suffix array's order is the order
// tan_compare computes on the text, in two dependent loads instead of d / 8.
__device__ __forceinline__ int tan_compare_isa(const uint32_t *__restrict__ isa,
                                               uint64_t s, uint64_t d,
                                               uint64_t l, uint64_t r)
{
  const uint64_t q = isa[s + d]; // s + d <= n: d regular symbols follow s
  return q < l ? -1 : (q > r ? 1 : 0);
}

// ISA: window comparisons through the inverse suffix array (isa), else on
// the text
template <typename IDX, bool ISA, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_tan_extent(const DevIndex<IDX> ix, const uint32_t *__restrict__ isa,
             const POS *__restrict__ cand,
             uint64_t ncand, uint64_t searchlength,
             TandemUnit<POS> *__restrict__ unit,
             uint64_t *__restrict__ counts, POS *__restrict__ rights)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= ncand)
  {
    return;
  }
  const uint64_t p = (uint64_t) cand[t] + 1;
  // lcp values of 255 and more live in llv, sorted by index: one binary
  // search finds the entry of p, its neighbours in the table are the next
  // positions with such a value to the left and to the right (what the
  // reference's getexception cache does, kurtz-basic/accvirt.c:69-150).  A
  // depth below 255 needs no entry at all: a byte of 255 is "larger".
  // (Round 2: with vsa_evallcp at every step of the two walks the kernel took
  // 150 ms on the 3 Gbp probe, nearly all of it in these binary searches.)
  const uint32_t bytep = ix.lcp[p];
  uint64_t e0 = 0, d = bytep;
  if (bytep == 255)
  {
    uint64_t lo = 0, hi = ix.nllv;
    while (lo < hi)
    {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if ((uint64_t) ix.llv[2 * mid] < p)
      {
        lo = mid + 1;
      } else
      {
        hi = mid;
      }
    }
    e0 = lo;
    d = (uint64_t) ix.llv[2 * e0 + 1];
  }
  TandemUnit<POS> u;
  // (a depth of 2^32 and more is cut: see k_rep_extent)
  u.d = (uint32_t) (d < 0xFFFFFFFFull ? d : 0xFFFFFFFFull);
  u.a = 1;
  u.b = 0;
  u.w = 0;
  uint64_t count = 0, r = p;
  bool first = false;
  if (d >= searchlength)
  {
    uint64_t l = p - 1, v, e = e0;
    for (;; l--) // lcp[0] = 0 <= d
    {
      v = ix.lcp[l];
      if (v == 255 && bytep == 255)
      {
        v = (uint64_t) ix.llv[2 * (--e) + 1];
      }
      if (v <= d)
      {
        break;
      }
    }
    first = v < d; // else an earlier position names this interval
    if (first)
    {
      e = e0;
      while (r + 1 <= ix.n)
      {
        v = ix.lcp[r + 1];
        if (v == 255 && bytep == 255)
        {
          v = (uint64_t) ix.llv[2 * (++e) + 1];
        }
        if (v < d)
        {
          break;
        }
        r++;
      }
      if (r - l + 1 == 2)
      {
        const uint64_t s0 = ix.suf[l], s1 = ix.suf[r];
        const uint64_t lo = s0 < s1 ? s0 : s1, hi = s0 < s1 ? s1 : s0;
        if (lo + d == hi)
        {
          // a, w without a condition on the outcome: a unit that reports
          // nothing is never looked at again.  (With the assignments inside
          // `if (... && tan_reported())` hipcc 7.2 -O3 lost u.a in the
          // 64-bit instantiation: the register was reused for the address of
          // the symbol load and "restored" to the initial value.)
          u.a = (POS) lo;
          u.w = (POS) ~(POS) 0;
          count = tan_reported(ix, lo, d) ? 1 : 0;
        }
      } else
      {
        const uint64_t alpha = ix.suf[l];
        auto window = [&](uint64_t s) -> int {
          return ISA ? tan_compare_isa(isa, s, d, l, r)
                     : tan_compare(ix, s, alpha, d);
        };
        // a = first index whose window is >= the interval's string
        uint64_t lo = l, hi = r + 1;
        while (lo < hi)
        {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (window((uint64_t) ix.suf[mid]) < 0)
          {
            lo = mid + 1;
          } else
          {
            hi = mid;
          }
        }
        const uint64_t a = lo;
        if (a <= r && window((uint64_t) ix.suf[a]) == 0)
        {
          // b = last index whose window is alpha
          lo = a;
          hi = r + 1;
          while (lo + 1 < hi)
          {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (window((uint64_t) ix.suf[mid]) == 0)
            {
              lo = mid;
            } else
            {
              hi = mid;
            }
          }
          const uint64_t b = lo;
          // the witness of findmaxprefixlen (kurtz/findmaxpref.gen:1-96):
          // left end, right end, then midpoints until one lies in [a, b]
          uint64_t w;
          if (a == l)
          {
            w = l;
          } else if (b == r)
          {
            w = r;
          } else
          {
            uint64_t left = l, right = r;
            w = a; // the loop always meets [a, b] before the ends touch
            while (right > left + 1)
            {
              const uint64_t mid = (left + right) / 2;
              if (mid < a)
              {
                left = mid;
              } else if (mid > b)
              {
                right = mid;
              } else
              {
                w = mid;
                break;
              }
            }
          }
          for (uint64_t i = a; i <= b; i++)
          {
            count += tan_reported(ix, (uint64_t) ix.suf[i], d) ? 1 : 0;
          }
          u.a = (POS) a;
          u.b = (POS) b;
          u.w = (POS) w;
        }
      }
    }
  }
  unit[t] = u;
  counts[t] = count;
  rights[t] = (POS) r;
}

// sort keys of the intervals that report something: right end ascending, then
// deeper first, in as few bits as the batch needs (see k_rep_keys)
template <typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_tan_keys(const POS *__restrict__ rights,
           const TandemUnit<POS> *__restrict__ unit,
           const uint32_t *__restrict__ order, uint64_t n, unsigned int dbits,
           uint64_t *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t < n)
  {
    const uint32_t o = order[t];
    const uint64_t r = rights[o], d = unit[o].d;
    out[t] = (r << dbits) | (((1ull << dbits) - 1) - d);
  }
}

template <typename POS>
struct TandemDepth
{
  __device__ uint32_t operator()(const TandemUnit<POS> &u) const
  {
    return u.d;
  }
};

template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_tan_write(const DevIndex<IDX> ix, const uint32_t *__restrict__ order,
            uint64_t ncand, const TandemUnit<POS> *__restrict__ unit,
            const uint64_t *__restrict__ offsets,
            vsa_match *__restrict__ out)
{
  const uint64_t t = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (t >= ncand || offsets[t + 1] == offsets[t])
  {
    return;
  }
  const TandemUnit<POS> u = unit[order[t]];
  const uint64_t d = u.d;
  uint64_t slot = offsets[t];
  vsa_match m;
  m.length = d;
  m.querystart = 0;
  if (u.w == (POS) ~(POS) 0)
  {
    m.dbstart = u.a;
    m.queryseq = m.dbstart + d;
    out[slot] = m;
    return;
  }
  for (uint64_t i = u.w;; i--) // witness, then leftwards
  {
    const uint64_t v = ix.suf[i];
    if (tan_reported(ix, v, d))
    {
      m.dbstart = v;
      m.queryseq = v + d;
      out[slot++] = m;
    }
    if (i == u.a)
    {
      break;
    }
  }
  for (uint64_t i = (uint64_t) u.w + 1; i <= u.b; i++)
  {
    const uint64_t v = ix.suf[i];
    if (tan_reported(ix, v, d))
    {
      m.dbstart = v;
      m.queryseq = v + d;
      out[slot++] = m;
    }
  }
}

template <typename IDX, typename POS>
int run_tandems(const vsa_index *index, uint64_t searchlength,
                vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  const uint64_t n = index->n;
  DevBuf cand, unit, counts, keys, order, order2, offsets, temp, dcount,
      matches;
  uint64_t ncand = 0, total = 0;

  res->stats.searches = n;
  if (dcount.alloc(8))
  {
    return -100;
  }
  tall.start();
  if (lcp_select<false, POS>(ix.lcp, n,
                        (uint32_t) (searchlength < 255 ? searchlength : 255),
                        stream, cand, &ncand))
  {
    return -100;
  }
  res->stats.candidates = ncand;
  if (ncand >= 0xFFFFFFFFull)
  {
    VSA_ERROR("tandem repeats: %llu positions with lcp >= %llu: more than "
              "2^32 intervals are not supported",
              (unsigned long long) ncand, (unsigned long long) searchlength);
    return -3;
  }
  if (ncand > 0)
  {
    if (unit.alloc(ncand * sizeof(TandemUnit<POS>)) ||
        counts.alloc(ncand * 8) ||
        keys.alloc(ncand * sizeof(POS)) || order.alloc(ncand * 4) ||
        order2.alloc(ncand * 4) || offsets.alloc((ncand + 1) * 8))
    {
      return -100;
    }
    // VSA_TANDEM_ISA=1: window comparisons through the inverse suffix array
    // (made by the first call, 4 bytes per position) instead of the text
    const char *useisa = getenv("VSA_TANDEM_ISA");
    const uint32_t *isa = nullptr;
    // (its entries are 32 bits wide: texts below 2^32 symbols)
    if (useisa != nullptr && strcmp(useisa, "1") == 0 &&
        n + 1 < 0xFFFFFFFFull && tan_inverse<IDX>(index, &isa))
    {
      return -100;
    }
    tsearch.start();
    if (isa != nullptr)
    {
      k_tan_extent<IDX, true, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
          ix, isa, cand.as<POS>(), ncand, searchlength,
          unit.as<TandemUnit<POS>>(), counts.as<uint64_t>(), keys.as<POS>());
    } else
    {
      k_tan_extent<IDX, false, POS><<<gridfor(ncand), VSA_BLOCK, 0, stream>>>(
          ix, isa, cand.as<POS>(), ncand, searchlength,
          unit.as<TandemUnit<POS>>(), counts.as<uint64_t>(), keys.as<POS>());
    }
    tsearch.stop();
    VSA_HIP(hipGetLastError());
    // Only the intervals that report something go on: of the 1.8e8 positions
    // of the 3 Gbp probe 2.8e6 (sorting all of them was 12 of its 50 ms).
    // order[] = their numbers, keysk[] their keys.  (Their number waits in
    // offsets[0] until it is fetched.)
    uint64_t nkeep = 0, maxd = 0;
    DevBuf keysk;
    auto reports = rocprim::make_transform_iterator(
        counts.as<uint64_t>(),
        [] __device__(uint64_t c) { return (uint8_t) (c != 0 ? 1 : 0); });
    VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
      return rocprim::select(p, tb, rocprim::counting_iterator<uint32_t>(0),
                             reports, order.as<uint32_t>(),
                             offsets.as<uint64_t>(), (size_t) ncand, stream);
    }));
    auto depth = rocprim::make_transform_iterator(unit.as<TandemUnit<POS>>(),
                                                  TandemDepth<POS>());
    VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
      return rocprim::reduce(p, tb, depth, dcount.as<uint32_t>(),
                             (uint32_t) 0, (size_t) ncand,
                             rocprim::maximum<uint32_t>(), stream);
    }));
    {
      const Fetch f[2] = {{dcount.p, 4}, {offsets.p, 8}};
      uint64_t got[2];
      if (fetchwords(stream, f, 2, got))
      {
        return -100;
      }
      maxd = got[0];
      nkeep = got[1];
    }
    if (nkeep > 0)
    {
      unsigned int dbits, endbit;
      if (keysk.alloc(nkeep * 8))
      {
        return -100;
      }
      if (keybits("tandem repeats", "unit", maxd, n, &dbits, &endbit))
      {
        return -3;
      }
      k_tan_keys<POS><<<gridfor(nkeep), VSA_BLOCK, 0, stream>>>(
          keys.as<POS>(), unit.as<TandemUnit<POS>>(), order.as<uint32_t>(),
          nkeep, dbits, keysk.as<uint64_t>());
      VSA_HIP(hipGetLastError());
      if (reportorder(keysk.as<uint64_t>(), order.as<uint32_t>(),
                      counts.as<uint64_t>(), nkeep, endbit,
                      order2.as<uint32_t>(), offsets.as<uint64_t>(), stream,
                      &total))
      {
        return -100;
      }
    }
    if (total > 0)
    {
      if (matches.alloc(total * sizeof(vsa_match)))
      {
        return -100;
      }
      k_tan_write<IDX, POS><<<gridfor(nkeep), VSA_BLOCK, 0, stream>>>(
          ix, order2.as<uint32_t>(), nkeep, unit.as<TandemUnit<POS>>(),
          offsets.as<uint64_t>(), matches.as<vsa_match>());
      VSA_HIP(hipGetLastError());
    }
  }
  return finish(res, matches, total, tall, tsearch, stream);
}
