// K4s: MUM candidates thrown into dbstart buckets, every bucket sorted AND
// filtered in LDS -- kernels and their host driver; included by esa_search.hip
// behind mum_filter.inc, whose rule (vsa_mum_alone_in_run) and scans it uses.
//
// The rule asks for the (key, value) pairs in order of dbstart = key >>
// lenbits, in ANY order inside a run of equal dbstarts -- runs are looked at as
// runs, and the order the candidates arrive in (wavefront atomics on cursor
// regions) differs from call to call anyway, so no stability either.  Four
// onesweep passes over 8-bit digits deliver more than that, and each pays a
// look-back chain over ~1 400 workgroups whatever it moves.  Candidates are
// positions spread over the text, so here they are
//
//   k_cs_scatter  thrown into buckets by the high bits of dbstart (bucket =
//                 dbstart >> shift, monotone in dbstart): a workgroup counts
//                 its tile of candidates per bucket in LDS, reserves its
//                 share of each bucket with one atomic on the bucket's
//                 counter, and ONE store per candidate puts the pair into the
//                 bucket's staging region (capacity VSA_CS_CAP).  Read
//                 straight from where candidates are produced: the cursor
//                 regions of the search kernel and of the plan, and the first
//                 pass's arrays, key and value formed as k_append_first forms
//                 them -- the dense list of compact() is never made here.
//                 A candidate whose right end lies in a later bucket leaves
//                 it there (atomicMax on bcarry[], one candidate in some
//                 thousands): bcarry[b] is all that bucket b has to know of
//                 the buckets in front of it, see k_cs_filter.
//   k_cs_filter   a workgroup per bucket: the bucket's pairs in registers, a
//                 counting sort in LDS on the top VSA_CS_BINBITS bits of the
//                 `shift` low dbstart bits (about one pair per bin), ranks
//                 inside a bin by looking at the bin, the pairs stored at
//                 their ranks; then the filter's rule on the sorted bucket
//                 where it lies, and the survivors written back in order to
//                 the front of the bucket's own staging region, with their
//                 number and the sum of their lengths.
//   k_mumf_scan   (mum_filter.inc) survivors per bucket -> where each
//                 bucket's records go; a second workgroup sums the lengths.
//   k_cs_write    a workgroup per bucket: its survivors from staging as
//                 32-byte records at the bucket's place in the result.
//
// Inside a bucket the high dbstart bits are implied by the place, so where
// shift + lenbits + 32 value bits fit into 64 a staging entry is 8 bytes
// (the headline: 19 + 7 + 32); otherwise key and value travel as one 16-byte
// store (64-bit values, or a text so long / a list so short that shift +
// lenbits > 32).
//
// Until round 12 the sorted pairs were written out as two arrays and read
// back by the five launches of mumfilter_tiles (tile maxima, scan, flags,
// scan, writer: 940 MB for the 11.6 M candidates of the headline batch where
// this moves 630).
//
// When it does not apply: candidates concentrated on a small part of the text
// (amplicon reads, a repeat family) overflow a bucket or, inside a bucket
// that fits, a bin: the ranking inside a bin is quadratic, so k_cs_filter
// gives up on a bin of more than VSA_CS_BINLIMIT pairs.  Either way the
// workgroup that sees it raises VSA_CS_OVERFLOW and leaves no survivors; then
// nothing is lost but time: the flag comes back with the counts, and the
// caller runs compact() and the rocPRIM sort as before.  The other workgroups
// and the writer go on in that case: wasted but safe (every per-bucket number
// is zeroed in front of the scatter, the loops are bounded by VSA_RUN_LIMIT,
// every index by VSA_CS_CAP, the bucket's count or the number of
// candidates), and the caller backs off on an index whose batches keep doing
// this (vsa_index::cs_skip).  A run of more than VSA_RUN_LIMIT equal dbstarts
// raises bit 0 (vsa_mum_alone_in_run), and the caller sorts on all bits.
//
// Measured on MI355X: profiles/r05/ (probe of the scatter, the sort alone)
// and profiles/r12/ (sort and filter in one kernel); DESIGN.md section 5
// quotes from there.

#define VSA_CS_CAP 4096 // pairs per bucket: 32 KB (64 KB) of LDS in k_cs_filter
#define VSA_CS_ITEMS (VSA_CS_CAP / VSA_BLOCK)
#define VSA_CS_BINBITS 11
#define VSA_CS_BINS (1u << VSA_CS_BINBITS)
// pairs a bin may hold: 256 LDS reads per pair at most in the ranking.  (A
// run of up to VSA_RUN_LIMIT = 64 equal dbstarts, which the filter's first
// attempt accepts, fits several times.)
#define VSA_CS_BINLIMIT 256
// bit of the filter's flag word (bit 0: "a run was too long",
// vsa_mum_alone_in_run)
#define VSA_CS_OVERFLOW 2u

struct CsGeometry
{
  unsigned int shift, lenbits; // bucket = (key >> lenbits) >> shift
  uint64_t nbuckets;
};

// a set of VSA_CURSOR_SHARDS cursor regions (keys == nullptr: none)
struct CsRegions
{
  const void *vals; // VAL per candidate
  const uint64_t *keys;
  const unsigned long long *cursors; // one per VSA_CURSOR_STRIDE words
  uint64_t cap;
  uint64_t total; // candidates in all regions (host: sizes the tiles)
};

// the first pass's candidates (fmlen == nullptr: none): read q is one iff
// fmlen[q] != 0
struct CsFirst
{
  const uint32_t *fmlen;
  const uint64_t *fmdb;
  uint64_t nq, seqoffset;
  uint32_t packbits, valbits;
};

struct CsSources
{
  CsRegions reg[2];
  CsFirst first;
};

// staging entries: SMALL = 8 bytes, (low shift + lenbits bits of the key)
// << 32 | value; else {key, value}
template <typename VAL, bool SMALL>
struct CsForm
{
  using Entry = typename std::conditional<SMALL, uint64_t, ulonglong2>::type;

  static __device__ __forceinline__ Entry make(uint64_t key, VAL val,
                                               const CsGeometry &g)
  {
    if constexpr (SMALL)
    {
      const uint64_t low = key & ((1ull << (g.shift + g.lenbits)) - 1);
      return (low << 32) | (uint64_t) val;
    } else
    {
      return make_ulonglong2(key, (uint64_t) val);
    }
  }
  // the `shift` low bits of dbstart
  static __device__ __forceinline__ uint64_t sub(const Entry &e,
                                                 const CsGeometry &g)
  {
    if constexpr (SMALL)
    {
      return e >> (32 + g.lenbits);
    } else
    {
      return (e.x >> g.lenbits) & ((1ull << g.shift) - 1);
    }
  }
  static __device__ __forceinline__ uint64_t key(const Entry &e,
                                                 uint64_t bucket,
                                                 const CsGeometry &g)
  {
    if constexpr (SMALL)
    {
      return (bucket << (g.shift + g.lenbits)) | (e >> 32);
    } else
    {
      return e.x;
    }
  }
  static __device__ __forceinline__ VAL val(const Entry &e)
  {
    if constexpr (SMALL)
    {
      return (VAL) e;
    } else
    {
      return (VAL) e.y;
    }
  }
};

// Which candidates a workgroup of k_cs_scatter takes: workgroups [0,
// ngroups[0]) group[0] consecutive cursor regions of the first set each, the
// next ngroups[1] group[1] regions of the second set, the ones behind them
// VSA_CS_TILE consecutive reads of the first pass
struct CsTiles
{
  uint32_t group[2], ngroups[2];
};

#define VSA_CS_SCATTER_BLOCK 1024
#define VSA_CS_TILE_ITEMS 8
#define VSA_CS_TILE (VSA_CS_SCATTER_BLOCK * VSA_CS_TILE_ITEMS)
// counters of a scatter workgroup in LDS (48 KB)
#define VSA_CS_MAXBUCKETS 12288

// fn(key, value) for every candidate in this workgroup's cursor regions
// (workgroup wg of the set's ngroups): a wavefront per region, so `group` is
// at most VSA_CS_SCATTER_BLOCK / 64.  (All wavefronts on one region after the
// other made a short list wait for up to 2 048 dependent cursor loads, several
// times what rocPRIM takes for such a list.)
template <typename VAL, typename Fn>
__device__ __forceinline__ void
vsa_cs_foreach(const CsRegions &r, uint64_t wg, uint32_t group, Fn fn)
{
  const VAL *vals = static_cast<const VAL *>(r.vals);
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint64_t shard = wg * group + wave;
  if (wave >= group || shard >= VSA_CURSOR_SHARDS)
  {
    return;
  }
  uint64_t count = r.cursors[shard * VSA_CURSOR_STRIDE];
  count = count < r.cap ? count : r.cap;
  const uint64_t at = shard * r.cap;
  for (uint64_t i = lane; i < count; i += 64)
  {
    fn(r.keys[at + i], vals[at + i]);
  }
}

// The scatter.  A returning atomicAdd per candidate on its bucket's counter
// in memory is what the probe rules out: every lane's atomic leaves the CU
// as a request of its own, and the device takes about 20 G of them per
// second -- for the 11.6 M candidates of the headline batch more than the
// sort it replaces, and more than three times what the stores alone take
// (profiles/r05/scatter_probe.txt).  So a workgroup
// takes a tile of candidates, counts them per bucket in LDS, reserves its
// share of every bucket it met with ONE atomic per bucket (a wavefront's 64
// counters are four 64-byte lines) and ranks its candidates by LDS atomics on
// the reserved starts.  The reads of the first pass -- five candidates of
// six in the headline batch -- are loaded once, eight per thread and all at
// once, and wait in registers (a workgroup that walked 32 reads per thread
// one load after the other, twice, took twice as long); the cursor regions
// are walked twice.
//
// bcarry[b] = the largest right end of a candidate of an earlier bucket that
// reaches into bucket b (0: none).  That is the reference's running `dbright`
// on entering b as far as it matters there: a candidate of b ends at or
// behind the start of b, and whatever does not reach b ends in front of it.
// With shift >= lenbits a candidate reaches one later bucket at most; a long
// match over narrow buckets (shift < lenbits) marks each one it reaches.
template <typename VAL, bool SMALL>
__global__ void __launch_bounds__(VSA_CS_SCATTER_BLOCK)
k_cs_scatter(CsSources src, CsTiles t, CsGeometry g,
             uint32_t *__restrict__ counts,
             unsigned long long *__restrict__ bcarry,
             typename CsForm<VAL, SMALL>::Entry *__restrict__ staging)
{
  extern __shared__ uint32_t cs_hist[]; // nbuckets words
  const KeyToRightEnd rightend = {g.lenbits};
  const uint32_t nb = (uint32_t) g.nbuckets;
  auto bucket = [&](uint64_t key) {
    const uint64_t b = (key >> g.lenbits) >> g.shift;
    return (uint32_t) (b < nb ? b : nb - 1); // (a dbstart beyond the text)
  };
  // (where all lanes that come here together bring the same bucket -- reads
  // cut from one window, the input that overflows -- the first of them adds
  // for all: 8 192 LDS atomics of a workgroup on one address, one after the
  // other, cost such a batch more than its whole rocPRIM sort)
  const uint32_t lane = threadIdx.x & 63u;
  auto count = [&](uint64_t key, VAL) {
    const uint32_t b = bucket(key);
    const uint64_t active = __ballot(1);
    const uint32_t b0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) b);
    if (__ballot(b == b0) == active)
    {
      if ((int) lane == __ffsll((unsigned long long) active) - 1)
      {
        atomicAdd(&cs_hist[b0], (uint32_t) __popcll(active));
      }
    } else
    {
      atomicAdd(&cs_hist[b], 1u);
    }
  };
  auto place = [&](uint64_t key, VAL val) {
    const uint32_t b = bucket(key);
    const uint64_t active = __ballot(1);
    const uint32_t b0 = (uint32_t) __builtin_amdgcn_readfirstlane((int) b);
    uint32_t rank;
    if (__ballot(b == b0) == active)
    {
      uint32_t base = 0;
      if ((int) lane == __ffsll((unsigned long long) active) - 1)
      {
        base = atomicAdd(&cs_hist[b0], (uint32_t) __popcll(active));
      }
      rank = (uint32_t) __builtin_amdgcn_readfirstlane((int) base) +
             (uint32_t) __popcll(active & ((1ull << lane) - 1));
    } else
    {
      rank = atomicAdd(&cs_hist[b], 1u);
    }
    if (rank < VSA_CS_CAP) // (beyond: counted, and k_cs_filter raises the
    {                      // flag)
      staging[(uint64_t) b * VSA_CS_CAP + rank] =
          CsForm<VAL, SMALL>::make(key, val, g);
    }
    const uint64_t end = rightend(key);
    uint64_t last = end >> g.shift;
    last = last < nb ? last : nb - 1;
    for (uint64_t later = (uint64_t) b + 1; later <= last; later++)
    {
      atomicMax(&bcarry[later], (unsigned long long) end);
    }
  };
  // which tile
  uint64_t wg = vsa_bid();
  int set = 0;
  while (set < 2 && wg >= t.ngroups[set])
  {
    wg -= t.ngroups[set++];
  }
  // a tile of the first pass: keys as k_append_first makes them, bit u of
  // `have`: read u of this thread is a candidate
  const CsFirst &f = src.first;
  uint64_t key[VSA_CS_TILE_ITEMS];
  uint32_t have = 0;
  const uint64_t q0 = wg * VSA_CS_TILE + threadIdx.x;
  if (set == 2)
  {
    uint32_t len[VSA_CS_TILE_ITEMS];
#pragma unroll
    for (int u = 0; u < VSA_CS_TILE_ITEMS; u++)
    {
      const uint64_t q = q0 + (uint64_t) u * VSA_CS_SCATTER_BLOCK;
      len[u] = q < f.nq ? f.fmlen[q] : 0;
      key[u] = q < f.nq ? f.fmdb[q] : 0;
    }
#pragma unroll
    for (int u = 0; u < VSA_CS_TILE_ITEMS; u++)
    {
      key[u] = (key[u] << f.packbits) | (((1ull << f.packbits) - 1) - len[u]);
      have |= len[u] != 0 ? 1u << u : 0u;
    }
  }
  for (uint32_t b = threadIdx.x; b < nb; b += VSA_CS_SCATTER_BLOCK)
  {
    cs_hist[b] = 0;
  }
  __syncthreads();
  if (set == 2)
  {
#pragma unroll
    for (int u = 0; u < VSA_CS_TILE_ITEMS; u++)
    {
      if ((have >> u) & 1u)
      {
        count(key[u], 0);
      }
    }
  } else
  {
    vsa_cs_foreach<VAL>(set == 0 ? src.reg[0] : src.reg[1], wg, t.group[set],
                        count);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += VSA_CS_SCATTER_BLOCK)
  {
    const uint32_t c = cs_hist[b];
    if (c != 0)
    {
      cs_hist[b] = atomicAdd(&counts[b], c);
    }
  }
  __syncthreads();
  if (set == 2)
  {
#pragma unroll
    for (int u = 0; u < VSA_CS_TILE_ITEMS; u++)
    {
      if ((have >> u) & 1u)
      {
        const uint64_t q = q0 + (uint64_t) u * VSA_CS_SCATTER_BLOCK;
        place(key[u], sizeof(VAL) == 4 ? (VAL) (q << f.valbits)
                                       : (VAL) ((q + f.seqoffset) << 16));
      }
    }
  } else
  {
    vsa_cs_foreach<VAL>(set == 0 ? src.reg[0] : src.reg[1], wg, t.group[set],
                        place);
  }
}

// A workgroup per bucket: its pairs sorted on the `shift` low dbstart bits in
// LDS, filtered there by the rule (vsa_mum_alone_in_run), and the survivors
// written back in order to the front of the bucket's staging region --
// staging[b * VSA_CS_CAP + i], i < bsurv[b]; blen[b] = the sum of their
// lengths.  (The workgroup owns the region and has read all of it into
// registers long before it writes.)  carry: see mumfilter_tiles.
//
// The sorted bucket is walked in rows of VSA_BLOCK, one pair per thread, so
// that LDS is read without bank conflicts.  A row of a wavefront is a
// segment: the running maximum of the right ends is scanned inside segments
// by shuffles, the (at most 64) segment maxima by the first wavefront, and
// the same two levels -- a ballot inside the segment -- place the survivors.
// The segments' words and the scans' lie in `bins`, which the sort needs no
// longer by then: 40 960 bytes of LDS in the 8-byte form are four workgroups
// per CU, one word more would be three.
template <typename VAL, bool SMALL>
__global__ void __launch_bounds__(VSA_BLOCK)
k_cs_filter(typename CsForm<VAL, SMALL>::Entry *__restrict__ staging,
            const uint32_t *__restrict__ counts,
            const unsigned long long *__restrict__ bcarry,
            unsigned int *__restrict__ flag, CsGeometry g, uint64_t carry,
            uint64_t *__restrict__ bsurv, uint64_t *__restrict__ blen)
{
  using F = CsForm<VAL, SMALL>;
  using Entry = typename F::Entry;
  constexpr uint32_t SEGS = VSA_CS_ITEMS * (VSA_BLOCK / 64);
  static_assert(SEGS <= 64, "the first wavefront scans the segments");
  __shared__ Entry buf[VSA_CS_CAP];
  __shared__ uint64_t binwords[VSA_CS_BINS / 2];
  uint32_t *bins = reinterpret_cast<uint32_t *>(binwords);
  // (the first scan's few words lie in buf, which is filled behind that scan)
  uint64_t *sh = reinterpret_cast<uint64_t *>(buf);
  // ("a bin is too large", in buf as well, behind the scan's words)
  uint32_t *toobig = reinterpret_cast<uint32_t *>(buf) + 32;
  const uint64_t b = vsa_bid();
  if (b >= g.nbuckets)
  {
    return;
  }
  const uint32_t c = counts[b];
  if (c == 0)
  {
    return;
  }
  if (c > VSA_CS_CAP) // (the scatter kept VSA_CS_CAP of them)
  {
    if (threadIdx.x == 0)
    {
      atomicOr(flag, VSA_CS_OVERFLOW);
    }
    return;
  }
  // An overflow: the list is sorted again by the caller, nothing to do here.
  // Workgroups of this very launch raise the flag, so the wavefronts of a
  // workgroup could read different values: one thread reads it, and all
  // decide on that word behind the barrier -- a workgroup goes on whole or
  // not at all.
  if (threadIdx.x == 0)
  {
    *toobig = (*flag & VSA_CS_OVERFLOW) != 0 ? 1u : 0u;
  }
  const unsigned int binshift =
      g.shift > VSA_CS_BINBITS ? g.shift - VSA_CS_BINBITS : 0;
  for (uint32_t k = threadIdx.x; k < VSA_CS_BINS; k += VSA_BLOCK)
  {
    bins[k] = 0;
  }
  __syncthreads();
  if (*toobig != 0) // (not written again before the next barrier but one)
  {
    return;
  }
  // the pairs of the bucket in registers; pairs per bin.  (A pair with
  // dbstart bits beyond the bucket -- none comes from the scatter -- counts
  // for the last bin: every index into bins stays below VSA_CS_BINS.)
  auto binof = [&](const Entry &x) {
    const uint64_t bin = F::sub(x, g) >> binshift;
    return (uint32_t) (bin < VSA_CS_BINS ? bin : VSA_CS_BINS - 1);
  };
  {
    Entry e[VSA_CS_ITEMS];
#pragma unroll
    for (int k = 0; k < VSA_CS_ITEMS; k++)
    {
      const uint32_t i = k * VSA_BLOCK + threadIdx.x;
      if (i < c)
      {
        e[k] = staging[b * VSA_CS_CAP + i];
        atomicAdd(&bins[binof(e[k])], 1u);
      }
    }
    __syncthreads();
    // bins[x] = pairs in the bins in front of x (a thread takes 8 bins)
    constexpr int PER = VSA_CS_BINS / VSA_BLOCK;
    {
      uint32_t v[PER];
      uint64_t mine = 0;
#pragma unroll
      for (int j = 0; j < PER; j++)
      {
        v[j] = bins[threadIdx.x * PER + j];
        mine += v[j];
      }
      uint64_t total;
      uint32_t ex = (uint32_t) vsa_block_exscan<0>(mine, sh, total);
#pragma unroll
      for (int j = 0; j < PER; j++)
      {
        bins[threadIdx.x * PER + j] = ex;
        ex += v[j];
      }
    }
    __syncthreads();
    // a bin too large for the quadratic ranking below: the caller sorts again
    uint32_t big = 0;
#pragma unroll
    for (int j = 0; j < PER; j++)
    {
      const uint32_t x = threadIdx.x * PER + j;
      const uint32_t end = x + 1 < VSA_CS_BINS ? bins[x + 1] : c;
      big |= end - bins[x] > VSA_CS_BINLIMIT ? 1u : 0u;
    }
    if (big != 0)
    {
      *toobig = 1;
    }
    __syncthreads();
    if (*toobig != 0) // (the same for every thread: read behind a barrier)
    {
      if (threadIdx.x == 0)
      {
        atomicOr(flag, VSA_CS_OVERFLOW);
      }
      return;
    }
    __syncthreads(); // (buf is written from here on)
    // into LDS bin by bin; afterwards bins[x] = the END of bin x
#pragma unroll
    for (int k = 0; k < VSA_CS_ITEMS; k++)
    {
      const uint32_t i = k * VSA_BLOCK + threadIdx.x;
      if (i < c)
      {
        const uint32_t at = atomicAdd(&bins[binof(e[k])], 1u);
        if (at < c) // (always)
        {
          buf[at] = e[k];
        }
      }
    }
  }
  __syncthreads();
  // the place of a pair inside its bin: the pairs of the bin with a smaller
  // dbstart, and those with the same one that lie in front of it.  Pairs and
  // places wait in registers until every thread has looked at its bins; then
  // buf is in dbstart order without a second buffer.
  {
    Entry m[VSA_CS_ITEMS];
    uint32_t place[VSA_CS_ITEMS];
#pragma unroll
    for (int k = 0; k < VSA_CS_ITEMS; k++)
    {
      const uint32_t p = k * VSA_BLOCK + threadIdx.x;
      place[k] = VSA_CS_CAP;
      if (p < c)
      {
        m[k] = buf[p];
        const uint64_t sm = F::sub(m[k], g);
        const uint32_t x = binof(m[k]);
        uint32_t first = x > 0 ? bins[x - 1] : 0, end = bins[x];
        end = end < c ? end : c; // (already so)
        uint32_t r = first;
        for (uint32_t j = first; j < end; j++)
        {
          const uint64_t sj = F::sub(buf[j], g);
          r += (sj < sm || (sj == sm && j < p)) ? 1u : 0u;
        }
        place[k] = r;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VSA_CS_ITEMS; k++)
    {
      if (place[k] < c) // (always for a pair there is; keeps the stores
      {                 // inside the bucket whatever LDS held)
        buf[place[k]] = m[k];
      }
    }
  }
  __syncthreads();
  // ---- the filter (bins is free from here on)
  uint64_t *segmax = binwords;       // SEGS words
  uint32_t *segcount = bins + 128;   // SEGS + 1 words
  uint64_t *sh2 = binwords + 128;    // a scan's few words
  const KeyToRightEnd rightend = {g.lenbits};
  const uint64_t lenmask = (1ull << g.lenbits) - 1;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nsegs = (c + VSA_BLOCK - 1) / VSA_BLOCK * (VSA_BLOCK / 64);
  auto keyat = [&](uint32_t i) { return F::key(buf[i], b, g); };
  // the largest right end in front of each pair inside its segment
  uint64_t before[VSA_CS_ITEMS];
#pragma unroll
  for (int r = 0; r < VSA_CS_ITEMS; r++)
  {
    before[r] = 0;
    if ((uint32_t) r * VSA_BLOCK < c) // (the same for the whole workgroup)
    {
      const uint32_t i = r * VSA_BLOCK + threadIdx.x;
      const uint64_t incl =
          vsa_wave_inclusive_scan<1>(i < c ? rightend(keyat(i)) : 0);
      before[r] = vsa_wave_exclusive(incl);
      if (lane == 63)
      {
        segmax[r * (VSA_BLOCK / 64) + wave] = incl;
      }
    }
  }
  __syncthreads();
  // ... and in front of each segment: the caller's carry, what reaches in
  // from the buckets in front, the segments in front
  if (threadIdx.x < 64)
  {
    const uint64_t mine = vsa_wave_exclusive(vsa_wave_inclusive_scan<1>(
        lane < nsegs ? segmax[lane] : 0));
    uint64_t start = bcarry[b];
    start = carry > start ? carry : start;
    segmax[lane] = mine > start ? mine : start;
  }
  __syncthreads();
  // who survives
  uint32_t okbits = 0;
  uint64_t len = 0;
#pragma unroll
  for (int r = 0; r < VSA_CS_ITEMS; r++)
  {
    if ((uint32_t) r * VSA_BLOCK < c)
    {
      const uint32_t i = r * VSA_BLOCK + threadIdx.x;
      bool ok = false;
      uint64_t kk = 0;
      if (i < c)
      {
        kk = keyat(i);
        const uint64_t e = rightend(kk);
        const uint64_t seg = segmax[r * (VSA_BLOCK / 64) + wave];
        const uint64_t run = seg > before[r] ? seg : before[r];
        ok = run < e && vsa_mum_alone_in_run(keyat, g.lenbits, i, c,
                                             kk >> g.lenbits, e, flag);
      }
      const uint64_t mask = __ballot(ok);
      if (lane == 0)
      {
        segcount[r * (VSA_BLOCK / 64) + wave] = (uint32_t) __popcll(mask);
      }
      okbits |= ok ? 1u << r : 0u;
      len += ok ? lenmask - (kk & lenmask) : 0;
    }
  }
  __syncthreads();
  // segcount[s] = survivors in the segments in front of s; [SEGS]: all
  if (threadIdx.x < 64)
  {
    const uint32_t v = lane < nsegs ? segcount[lane] : 0;
    const uint32_t incl = vsa_wave_inclusive_scan<0>(v);
    segcount[lane] = incl - v;
    if (lane == 63)
    {
      segcount[SEGS] = incl;
    }
  }
  __syncthreads();
  // the survivors back into the bucket's region, in order: a survivor goes
  // to a place at or in front of the one it had in the sorted bucket
#pragma unroll
  for (int r = 0; r < VSA_CS_ITEMS; r++)
  {
    if ((uint32_t) r * VSA_BLOCK < c)
    {
      const bool ok = ((okbits >> r) & 1u) != 0;
      const uint64_t mask = __ballot(ok);
      const uint32_t at = segcount[r * (VSA_BLOCK / 64) + wave] +
                          (uint32_t) __popcll(mask & ((1ull << lane) - 1));
      if (ok && at < c) // (always)
      {
        staging[b * VSA_CS_CAP + at] = buf[r * VSA_BLOCK + threadIdx.x];
      }
    }
  }
  uint64_t alllen;
  (void) vsa_block_exscan<0>(len, sh2, alllen);
  if (threadIdx.x == 0)
  {
    const uint32_t kept = segcount[SEGS];
    bsurv[b] = kept < c ? kept : c; // (already so)
    blen[b] = alllen;
  }
}

// A workgroup per bucket: the bucket's survivors, which k_cs_filter left at
// the front of its staging region, as records at off[b] + i.  Walked in rows
// of VSA_BLOCK, one survivor per thread, so that the records of neighbouring
// lanes lie next to each other (see k_mumf_write).
template <typename VAL, bool SMALL>
__global__ void __launch_bounds__(VSA_BLOCK)
k_cs_write(const typename CsForm<VAL, SMALL>::Entry *__restrict__ staging,
           const uint64_t *__restrict__ bsurv, const uint64_t *__restrict__ off,
           CsGeometry g, uint64_t ncand, PairRecord<VAL> write,
           vsa_match *__restrict__ out)
{
  using F = CsForm<VAL, SMALL>;
  const uint64_t b = vsa_bid();
  if (b >= g.nbuckets)
  {
    return;
  }
  uint64_t n = bsurv[b];
  n = n < VSA_CS_CAP ? n : VSA_CS_CAP;
  const uint64_t at = off[b];
  // (at + n <= ncand, the records `out` has room for, unless the scatter met
  // more candidates than the caller knew of)
#pragma unroll 4
  for (uint64_t i = threadIdx.x; i < n; i += VSA_BLOCK)
  {
    if (at + i < ncand)
    {
      const typename F::Entry e = staging[b * VSA_CS_CAP + i];
      write(F::key(e, b, g), (uint64_t) F::val(e), out + at + i);
    }
  }
}

// bucket = dbstart >> shift with the largest shift that keeps the average
// bucket at or below half of VSA_CS_CAP (positions spread evenly: a Poisson
// count of 2 000 stays below 2 300 in every one of a million buckets); a list
// too short for two buckets is one bucket
inline CsGeometry cs_geometry(uint64_t textlen, uint64_t ncand,
                              unsigned int lenbits, unsigned int dbbits)
{
  CsGeometry g;
  const unsigned __int128 room =
      (unsigned __int128) (VSA_CS_CAP / 2) * ((unsigned __int128) textlen + 1);
  unsigned int s = 0;
  while (s < dbbits && s < 63 && ((unsigned __int128) ncand << (s + 1)) <= room)
  {
    s++;
  }
  g.shift = s;
  g.lenbits = lenbits;
  g.nbuckets = (textlen >> s) + 1;
  return g;
}

// The MUMs of the candidates of `src` (ncand of them, positions in a text of
// textlen symbols), as records in dbstart order in `out` (room for ncand):
// what rocprim::radix_sort_pairs(keys, k2, vals, v2, ncand, lenbits, lenbits
// + dbbits) and mumfilter_tiles<false>(..., carry, write, ...) deliver.
// got[] = their number, the sum of their lengths and the flag word (bit 0: a
// run was too long for the filter by runs, VSA_CS_OVERFLOW: a bucket or a bin
// did not fit); with a flag up the first two and `out` are not to be used.
// *used: the geometry it chose.
template <typename VAL>
int candidate_bucketfilter(const CsSources &src, uint64_t ncand,
                           uint64_t textlen, unsigned int lenbits,
                           unsigned int dbbits, uint64_t carry,
                           PairRecord<VAL> write, hipStream_t stream,
                           vsa_match *out, uint64_t got[3], CsGeometry *used)
{
  const CsGeometry g = cs_geometry(textlen, ncand, lenbits, dbbits);
  if (g.nbuckets > VSA_CS_MAXBUCKETS) // (the caller asks cs_geometry first)
  {
    return -100;
  }
  const bool small = sizeof(VAL) == 4 && g.shift + lenbits <= 32;
  // One allocation of 8-byte words.  What has to be zero lies in front and is
  // zeroed by one fill: the flag word (with a word of padding), bcarry,
  // survivors and their lengths per bucket, the buckets' counters (4 bytes
  // each), in whole 16 bytes.  Behind it what the scan writes: offsets and running lengths, one
  // more than buckets each.
  const uint64_t nb = g.nbuckets;
  const uint64_t zeroed = (2 + 3 * nb + (nb + 1) / 2 + 1) & ~1ull;
  DevBuf words, staging;
  if (words.alloc((zeroed + 2 * (nb + 1)) * 8) ||
      staging.alloc(nb * VSA_CS_CAP * (small ? 8 : 16)))
  {
    return -100;
  }
  uint64_t *w = words.as<uint64_t>();
  unsigned int *flag = reinterpret_cast<unsigned int *>(w);
  unsigned long long *bcarry = reinterpret_cast<unsigned long long *>(w + 2);
  uint64_t *bsurv = w + 2 + nb, *blen = w + 2 + 2 * nb;
  uint32_t *counts = reinterpret_cast<uint32_t *>(w + 2 + 3 * nb);
  uint64_t *off = w + zeroed, *lenscan = off + nb + 1;
  VSA_HIP(hipMemsetAsync(w, 0, zeroed * 8, stream));
  // cursor regions in groups of about a tile's worth of candidates
  CsTiles t = CsTiles();
  uint64_t nwg = 0;
  for (int s = 0; s < 2; s++)
  {
    if (src.reg[s].keys != nullptr)
    {
      const uint64_t per = src.reg[s].total / VSA_CURSOR_SHARDS + 1;
      t.group[s] = (uint32_t) std::min<uint64_t>(
          std::max<uint64_t>(VSA_CS_TILE / per, 1), VSA_CS_SCATTER_BLOCK / 64);
      t.ngroups[s] = (VSA_CURSOR_SHARDS + t.group[s] - 1) / t.group[s];
      nwg += t.ngroups[s];
    }
  }
  if (src.first.fmlen != nullptr)
  {
    nwg += (src.first.nq + VSA_CS_TILE - 1) / VSA_CS_TILE;
  }
  const dim3 sg = vsa_grid(nwg), bg = vsa_grid(nb);
  auto run = [&](auto sm) {
    using F = CsForm<VAL, decltype(sm)::value>;
    using Entry = typename F::Entry;
    k_cs_scatter<VAL, decltype(sm)::value>
        <<<sg, VSA_CS_SCATTER_BLOCK, nb * 4, stream>>>(
            src, t, g, counts, bcarry, staging.as<Entry>());
    k_cs_filter<VAL, decltype(sm)::value><<<bg, VSA_BLOCK, 0, stream>>>(
        staging.as<Entry>(), counts, bcarry, flag, g, carry, bsurv, blen);
    // (offsets of the buckets and, in a second workgroup, the sum of the
    // lengths)
    k_mumf_scan<0><<<2, VSA_BLOCK, 0, stream>>>(bsurv, nb, 0, off, blen,
                                                lenscan);
    k_cs_write<VAL, decltype(sm)::value><<<bg, VSA_BLOCK, 0, stream>>>(
        staging.as<Entry>(), bsurv, off, g, ncand, write, out);
  };
  if constexpr (sizeof(VAL) == 4)
  {
    if (small)
    {
      run(std::true_type());
    } else
    {
      run(std::false_type());
    }
  } else
  {
    run(std::false_type());
  }
  VSA_HIP(hipGetLastError());
  const Fetch f[3] = {{off + nb, 8}, {lenscan + nb, 8}, {flag, 8}};
  if (fetchwords(stream, f, 3, got))
  {
    return -100;
  }
  *used = g;
  return 0;
}
