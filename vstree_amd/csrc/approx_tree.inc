// Approximate complete matches, the configurations that reach esaapm /
// esahamming in the reference (Vmengine/splitesaapm.c:400-425, 523-543):
// pieces with a threshold of their own (K >= m/10) and patterns that are not
// cut at all (splitsize 1: short patterns).  Included by esa_search.hip
// behind approx_search.inc, whose region / verification kernels it reuses.
//
// esaapm (Vmengine/esaapm.c:296-383) and esahamming (esahamming.c:86-164) walk
// the suffixes in suffix array order with a stack of columns (mismatch
// counts) per depth and the skip table, and report every suffix for which
//   Hamming:  the first plen symbols exist, hold no separator and differ from
//             the pattern in at most t places (bytes: a wildcard equals a
//             wildcard), with the number of mismatches;
//   edit:     some prefix of at most min(plen + t, symbols left) symbols,
//             without a separator, is within t errors of the pattern (Eq masks
//             of getEqs4: a wildcard matches nothing) -- the walk stops at the
//             first such depth.
// Both conditions depend on a prefix of the suffix only, so the suffixes that
// satisfy them are whole lcp-intervals: here one work-item per pattern (or
// piece) descends the lcp-interval tree depth first -- children in the order
// a, c, g, t, then the suffixes whose next symbol is special, i.e. ascending
// suffix array order -- with the column of the current depth on a stack, and
// reports intervals [left, left + count).  A child interval is found by binary
// search on the symbol at the node's depth (two dependent reads per probe);
// nothing here is tuned: these searches visit a few hundred nodes and report
// thousands of positions per pattern, in the reference as well.
//
// Patterns that are not cut ("direct", splitsize 1) report straight to the
// output function in that order (edistprocessstartpos / hammingprocessstartpos,
// approxcompl.c:14-83); pieces feed the region tree exactly like exact piece
// hits do (storeapmposition, splitesaapm.c:268-302), and everything behind
// that -- merging, right-to-left verification, longest match -- is the code of
// approx_search.inc.  One deviation, in the last plen + t symbols of the
// whole text only: the reference reports a skipped suffix with the `maxlength`
// of the first suffix of its skipped run (esaapm.c:341-378) and lets the
// longest match read beyond the mapped text; here every suffix has its own
// maxlength and the text ends where it ends (the CPU restatement the tests
// use does the same).

#define VSA_TREE_MAXPLEN 32u // DPWORDSIZE4: pieces and uncut patterns
#define VSA_TREE_MAXDEPTH (2 * VSA_TREE_MAXPLEN + 1)

// (POS: 32 bits, 64 for suffix arrays of 2^32 entries and more)
template <typename POS>
struct TreeFrame
{
  POS l, r;        // suffix array interval of the node
  POS next;        // first suffix not yet handed to a child
  uint8_t child;   // next child to try: 0..3 regular symbols, 4 specials
  uint8_t mm;      // Hamming: mismatches so far
};

// rank of the symbol at depth d of suffix x: 0..3, 4 = special / behind the end
template <typename IDX>
__device__ __forceinline__ uint32_t tree_symbol(const DevIndex<IDX> &ix,
                                                uint64_t x, uint32_t d,
                                                uint8_t &raw)
{
  const uint64_t s = (uint64_t) ix.suf[x] + d;
  raw = s < ix.n ? ix.tis[s] : (uint8_t) VSA_SEPARATOR;
  return raw < 4 ? raw : 4u;
}

// One work-item per piece.  WRITE = false: counts[piece] = intervals;
// WRITE = true: writes them at offsets[piece].. in suffix array order.
template <typename IDX, bool EDIT, bool WRITE>
__global__ void __launch_bounds__(64)
k_apm_tree(const DevIndex<IDX> ix, const DevQueries qs, uint64_t npieces,
           const uint64_t *__restrict__ pstart,
           const uint64_t *__restrict__ plen,
           const uint32_t *__restrict__ pquery,
           const uint32_t *__restrict__ ppoffset,
           const uint32_t *__restrict__ qmode,
           uint64_t *__restrict__ counts,
           const uint64_t *__restrict__ offsets,
           uint64_t *__restrict__ ivleft, uint64_t *__restrict__ ivcount,
           uint32_t *__restrict__ ivvalue, uint32_t *__restrict__ ivquery,
           uint32_t *__restrict__ ivpoffset)
{
  const uint64_t p = vsa_bid() * 64 + threadIdx.x;
  if (p >= npieces)
  {
    return;
  }
  const uint8_t *pat = qs.symbols + pstart[p];
  const uint32_t m = (uint32_t) plen[p], q = pquery[p],
                 t = qmode[q] & 0x7FFFFFFFu;
  uint64_t found = 0, slot = WRITE ? offsets[p] : 0;
  if (m == 0 || m > VSA_TREE_MAXPLEN || ix.n == 0)
  {
    if (!WRITE)
    {
      counts[p] = 0;
    }
    return;
  }
  const uint32_t maxdepth = EDIT ? m + t : m;
  TreeFrame<IDX> st[VSA_TREE_MAXDEPTH + 1];
  // edit distance: the column of every depth on the path, cell by cell
  uint8_t col[EDIT ? VSA_TREE_MAXDEPTH + 1 : 1][EDIT ? VSA_TREE_MAXPLEN + 1 : 1];
  if (EDIT)
  {
    for (uint32_t i = 0; i <= m; i++)
    {
      col[0][i] = (uint8_t) i;
    }
  }
#define TREE_REPORT(L, C, V)                                                  \
  {                                                                           \
    if (WRITE)                                                                \
    {                                                                         \
      ivleft[slot] = (L);                                                     \
      ivcount[slot] = (C);                                                    \
      ivvalue[slot] = (V);                                                    \
      ivquery[slot] = q;                                                      \
      ivpoffset[slot] = ppoffset[p];                                          \
      slot++;                                                                 \
    }                                                                         \
    found++;                                                                  \
  }
  int sp = 0;
  st[0].l = 0;
  st[0].r = (IDX) (ix.n - 1); // suffixes 0 .. n-1 (suf[n] is the end)
  st[0].next = 0;
  st[0].child = 0;
  st[0].mm = 0;
  while (sp >= 0)
  {
    TreeFrame<IDX> &f = st[sp];
    const uint32_t d = (uint32_t) sp;
    if (f.child == 0 && f.next == f.l)
    {
      // first visit of the node: is the walk over here?
      if (EDIT)
      {
        if (col[d][m] <= t)
        {
          TREE_REPORT(f.l, (uint64_t) f.r - (uint64_t) f.l + 1, 0);
          sp--;
          continue;
        }
        if (d == maxdepth)
        {
          sp--;
          continue;
        }
      } else if (d == m)
      {
        TREE_REPORT(f.l, (uint64_t) f.r - (uint64_t) f.l + 1, f.mm);
        sp--;
        continue;
      }
    }
    if (f.next > f.r || f.child > 4)
    {
      sp--;
      continue;
    }
    const uint32_t c = f.child++;
    if (c < 4)
    {
      // the suffixes of [next, r] with symbol c at depth d: a prefix of it
      uint8_t raw;
      if (tree_symbol(ix, f.next, d, raw) != c)
      {
        continue; // (ranks ascend inside a node: none has c)
      }
      IDX lo = f.next, hi = f.r; // last index with rank <= c
      while (lo < hi)
      {
        const IDX mid = lo + (hi - lo + 1) / 2;
        if (tree_symbol(ix, mid, d, raw) <= c)
        {
          lo = mid;
        } else
        {
          hi = mid - 1;
        }
      }
      const IDX cl = f.next, cr = lo;
      f.next = cr + 1;
      TreeFrame<IDX> &g = st[sp + 1];
      if (EDIT)
      {
        // next column: the pattern against one more text symbol c
        uint32_t alive = 0;
        col[d + 1][0] = (uint8_t) (d + 1);
        alive |= (d + 1 <= t) ? 1u : 0u;
        for (uint32_t i = 1; i <= m; i++)
        {
          uint32_t v = col[d][i - 1] + ((pat[i - 1] == c) ? 0u : 1u);
          const uint32_t up = col[d + 1][i - 1] + 1u, we = col[d][i] + 1u;
          v = v < up ? v : up;
          v = v < we ? v : we;
          col[d + 1][i] = (uint8_t) (v > 250 ? 250 : v);
          alive |= (v <= t) ? 1u : 0u;
        }
        if (alive == 0)
        {
          continue; // no entry within the threshold: nothing below matches
        }
        g.mm = 0;
      } else
      {
        const uint32_t mm = f.mm + ((pat[d] == c) ? 0u : 1u);
        if (mm > t)
        {
          continue;
        }
        g.mm = (uint8_t) mm;
      }
      g.l = cl;
      g.r = cr;
      g.next = cl;
      g.child = 0;
      sp++;
      continue;
    }
    // c == 4: the suffixes of [next, r] have a special symbol (or the end of
    // the text) at depth d; every special symbol is unique, so each of them
    // is a leaf and is followed along the text on its own
    for (uint64_t x = f.next; x <= (uint64_t) f.r; x++)
    {
      const uint64_t s = (uint64_t) ix.suf[x];
      uint64_t vlen = ix.n - s;
      if (EDIT)
      {
        // columns d+1 .. along the text of this suffix
        uint8_t a[VSA_TREE_MAXPLEN + 1], b[VSA_TREE_MAXPLEN + 1];
        for (uint32_t i = 0; i <= m; i++)
        {
          a[i] = col[d][i];
        }
        const uint32_t maxlength =
            (uint64_t) maxdepth < vlen ? maxdepth : (uint32_t) vlen;
        bool ok = false;
        for (uint32_t e = d; e < maxlength; e++)
        {
          const uint8_t ch = ix.tis[s + e];
          if (ch == VSA_SEPARATOR)
          {
            break;
          }
          uint32_t alive = (e + 1 <= t) ? 1u : 0u;
          b[0] = (uint8_t) (e + 1);
          for (uint32_t i = 1; i <= m; i++)
          {
            // a wildcard matches nothing (getEqs4)
            uint32_t v = a[i - 1] +
                         ((pat[i - 1] == ch && ch != VSA_WILDCARD) ? 0u : 1u);
            const uint32_t up = b[i - 1] + 1u, we = a[i] + 1u;
            v = v < up ? v : up;
            v = v < we ? v : we;
            b[i] = (uint8_t) (v > 250 ? 250 : v);
            alive |= (v <= t) ? 1u : 0u;
          }
          if (b[m] <= t)
          {
            ok = true;
            break;
          }
          if (alive == 0)
          {
            break;
          }
          for (uint32_t i = 0; i <= m; i++)
          {
            a[i] = b[i];
          }
        }
        if (ok)
        {
          TREE_REPORT(x, 1, 0);
        }
      } else
      {
        uint32_t mm = f.mm;
        bool ok = vlen >= m;
        for (uint32_t e = d; ok && e < m; e++)
        {
          const uint8_t ch = ix.tis[s + e];
          if (ch == VSA_SEPARATOR || (ch != pat[e] && ++mm > t))
          {
            ok = false;
          }
        }
        if (ok)
        {
          TREE_REPORT(x, 1, mm);
        }
      }
    }
    sp--;
  }
#undef TREE_REPORT
  if (!WRITE)
  {
    counts[p] = found;
  }
}

// intervals of pieces feed the region tree, intervals of uncut patterns the
// output: split the counts
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_treesplit(const uint64_t *__restrict__ ivcount,
                const uint32_t *__restrict__ ivquery,
                const uint32_t *__restrict__ qmode, uint64_t nintervals,
                uint64_t *__restrict__ piececount,
                uint64_t *__restrict__ directcount)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < nintervals)
  {
    const bool direct = (qmode[ivquery[i]] >> 31) != 0;
    piececount[i] = direct ? 0 : ivcount[i];
    directcount[i] = direct ? ivcount[i] : 0;
  }
  if (i == nintervals)
  {
    piececount[i] = directcount[i] = 0;
  }
}

// one work-item per reported suffix of an uncut pattern, in output order.
// Hamming: the match itself (hammingprocessstartpos, approxcompl.c:68-83).
// Edit distance: the start position with a region of its own, [pos, pos +
// maxlength), for k_apm_longest (edistprocessstartpos, approxcompl.c:14-66).
template <typename IDX, typename POS>
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_directhits(const DevIndex<IDX> ix, const DevQueries qs,
                 const uint32_t *__restrict__ qk, uint64_t nintervals,
                 const uint64_t *__restrict__ ivleft,
                 const uint64_t *__restrict__ doffsets,
                 const uint32_t *__restrict__ ivvalue,
                 const uint32_t *__restrict__ ivquery, uint64_t ndirect,
                 bool doedist, vsa_match *__restrict__ out,
                 POS *__restrict__ hitpos,
                 uint32_t *__restrict__ hitregion, uint32_t *__restrict__ rq,
                 POS *__restrict__ rlo, POS *__restrict__ rhi)
{
  const uint64_t h = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (h >= ndirect)
  {
    return;
  }
  // the interval that holds hit h: last i with doffsets[i] <= h
  uint64_t lo = 0, hi = nintervals;
  while (hi - lo > 1)
  {
    const uint64_t mid = (lo + hi) >> 1;
    if (doffsets[mid] <= h)
    {
      lo = mid;
    } else
    {
      hi = mid;
    }
  }
  const uint32_t q = ivquery[lo];
  const uint64_t pos = (uint64_t) ix.suf[ivleft[lo] + (h - doffsets[lo])];
  const uint8_t *pattern;
  uint32_t m;
  apm_query(qs, q, pattern, m);
  if (!doedist)
  {
    vsa_match mt;
    mt.length = m;
    mt.dbstart = pos;
    mt.queryseq = (uint64_t) q + qs.seqoffset;
    mt.querystart = ivvalue[lo];
    out[h] = mt;
    return;
  }
  uint64_t maxlength = (uint64_t) m + qk[q];
  if (maxlength > ix.n - pos)
  {
    maxlength = ix.n - pos;
  }
  hitpos[h] = (POS) pos;
  hitregion[h] = (uint32_t) h;
  rq[h] = q;
  rlo[h] = (POS) pos;
  rhi[h] = (POS) (pos + maxlength - 1);
}

// keys for the final order: the matches of a query stay together and keep
// their order (every query is answered by one of the two paths)
__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_querykeys(const vsa_match *__restrict__ matches, uint64_t count,
                uint64_t seqoffset, uint32_t *__restrict__ keys,
                uint32_t *__restrict__ index)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < count)
  {
    keys[i] = (uint32_t) (matches[i].queryseq - seqoffset);
    index[i] = (uint32_t) i;
  }
}

__global__ void __launch_bounds__(VSA_BLOCK)
k_apm_gathermatches(const vsa_match *__restrict__ in,
                    const uint32_t *__restrict__ index, uint64_t count,
                    vsa_match *__restrict__ out)
{
  const uint64_t i = vsa_bid() * VSA_BLOCK + threadIdx.x;
  if (i < count)
  {
    out[i] = in[index[i]];
  }
}

// is this batch one for the tree path?  0: yes (plan filled), VSA_NOT_COVERED
// with a message: neither path takes it
struct TreePlan
{
  std::vector<uint32_t> k, splitlen, mode; // mode = piece threshold | direct << 31
  std::vector<uint64_t> piecebase;         // nq + 1
  uint64_t qlimit, failk, failm;
  uint32_t maxm;
};

static int apm_treeplan(const vsa_index *index, const vsa_queries *queries,
                        bool doedist, uint64_t distvalue, bool percent,
                        TreePlan &plan)
{
  const uint64_t nq = queries->nq;
  plan.qlimit = nq;
  plan.failk = plan.failm = 0;
  plan.maxm = 0;
  plan.k.assign(nq, 0);
  plan.splitlen.assign(nq, 0);
  plan.mode.assign(nq, 0);
  plan.piecebase.assign(nq + 1, 0);
  for (uint64_t q = 0; q < nq; q++)
  {
    const uint64_t m = queries->uniform ? queries->maxlength
                                        : queries->hlength[q];
    const uint64_t k = apm_explicitk != nullptr
                           ? apm_explicitk[q]
                           : (percent ? (m * distvalue) / 100 : distvalue);
    plan.piecebase[q + 1] = plan.piecebase[q];
    if (k == 0)
    {
      VSA_ERROR("a batch that mixes thresholds 0 and > 0 is not covered by "
                "the GPU engine");
      return VSA_NOT_COVERED;
    }
    if (k >= m)
    {
      plan.qlimit = q; // splitesaapm.c:496-501: the run stops here
      plan.failk = k;
      plan.failm = m;
      break;
    }
    if (m > 64 * VSA_APM_MAXWORDS)
    {
      VSA_ERROR("approximate search of query %lu (length %lu) is not covered "
                "by the GPU engine", (unsigned long) q, (unsigned long) m);
      return VSA_NOT_COVERED;
    }
    const uint64_t splitsize =
        apm_getoptsplit(doedist, 10, index->numofchars, index->n, m, k);
    const bool direct = splitsize <= 1;
    const uint64_t splitlen = direct ? m : m / splitsize,
                   st = direct ? k : k / splitsize;
    if (splitlen > VSA_TREE_MAXPLEN)
    {
      // (the reference: NOTIMPLEMENTED "large pattern after splitting";
      // cannot happen, getoptsplit keeps m <= 32 * splitsize)
      VSA_ERROR("approximate search: pieces of %lu symbols",
                (unsigned long) splitlen);
      return VSA_NOT_COVERED;
    }
    plan.k[q] = (uint32_t) k;
    plan.splitlen[q] = (uint32_t) splitlen;
    plan.mode[q] = (uint32_t) st | (direct ? 0x80000000u : 0u);
    plan.piecebase[q + 1] += m / splitlen;
    plan.maxm = std::max(plan.maxm, (uint32_t) m);
  }
  return 0;
}

// T1: what the tree search has found.  Interval i = the suffixes left[i] ..
// left[i] + count[i] - 1 of the suffix array, reported with value[i]
// (mismatches) for query[i], piece offset poffset[i].  The intervals of cut
// patterns feed the regions (poffsets: where their hits stand in that list,
// `total` hits), the ones of uncut patterns the output (doffsets, `ndirect`).
struct TreeIntervals
{
  uint64_t n = 0, total = 0, ndirect = 0;
  DevBuf mode, counts, offsets; // per query; per piece (+ 1)
  DevBuf left, count, value, query, poffset, poffsets, doffsets;
  int alloc(uint64_t nq, uint64_t npieces)
  {
    return (mode.alloc(nq * 4) || counts.alloc((npieces + 1) * 8) ||
            offsets.alloc((npieces + 1) * 8))
               ? -100
               : 0;
  }
};

// the lcp-interval tree, count pass then write pass (tsearch), and the split
// of the intervals into the two kinds
template <typename IDX>
int apm_treesearch(const DevIndex<IDX> &ix, const DevQueries &qs,
                   ApmPieces &pc, const std::vector<uint32_t> &mode,
                   uint64_t nq, uint64_t npieces, bool doedist,
                   Timer &tsearch, hipStream_t stream, TreeIntervals &iv)
{
  DevBuf pcount, dcount;
  const unsigned int tgrid = (unsigned int) ((npieces + 63) / 64);
  auto pass = [&](auto edit, auto write) {
    k_apm_tree<IDX, decltype(edit)::value, decltype(write)::value>
        <<<tgrid, 64, 0, stream>>>(
            ix, qs, npieces, pc.start.as<uint64_t>(), pc.len.as<uint64_t>(),
            pc.query.as<uint32_t>(), pc.poffset.as<uint32_t>(),
            iv.mode.as<uint32_t>(), iv.counts.as<uint64_t>(),
            iv.offsets.as<uint64_t>(), iv.left.as<uint64_t>(),
            iv.count.as<uint64_t>(), iv.value.as<uint32_t>(),
            iv.query.as<uint32_t>(), iv.poffset.as<uint32_t>());
    return hipGetLastError();
  };
  VSA_HIP(hipMemcpyAsync(iv.mode.p, mode.data(), nq * 4,
                         hipMemcpyHostToDevice, stream));
  tsearch.start();
  VSA_HIP(doedist ? pass(std::true_type(), std::false_type())
                  : pass(std::false_type(), std::false_type()));
  VSA_HIP(hipMemsetAsync(iv.counts.as<uint64_t>() + npieces, 0, 8, stream));
  if (exclusive_sum(iv.counts.as<uint64_t>(), iv.offsets.as<uint64_t>(),
                    npieces, stream, &iv.n))
  {
    return -100;
  }
  if (iv.n >= 0xFFFFFFFFull)
  {
    VSA_ERROR("approximate search: more than 2^32 intervals");
    return -5;
  }
  if (iv.n == 0)
  {
    tsearch.stop();
    return 0;
  }
  if (iv.left.alloc(iv.n * 8) || iv.count.alloc(iv.n * 8) ||
      iv.value.alloc(iv.n * 4) || iv.query.alloc(iv.n * 4) ||
      iv.poffset.alloc(iv.n * 4) || pcount.alloc((iv.n + 1) * 8) ||
      iv.poffsets.alloc((iv.n + 1) * 8) || dcount.alloc((iv.n + 1) * 8) ||
      iv.doffsets.alloc((iv.n + 1) * 8))
  {
    return -100;
  }
  VSA_HIP(doedist ? pass(std::true_type(), std::true_type())
                  : pass(std::false_type(), std::true_type()));
  tsearch.stop();
  k_apm_treesplit<<<gridfor(iv.n + 1), VSA_BLOCK, 0, stream>>>(
      iv.count.as<uint64_t>(), iv.query.as<uint32_t>(),
      iv.mode.as<uint32_t>(), iv.n, pcount.as<uint64_t>(),
      dcount.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  if (exclusive_sum(pcount.as<uint64_t>(), iv.poffsets.as<uint64_t>(), iv.n,
                    stream, &iv.total) ||
      exclusive_sum(dcount.as<uint64_t>(), iv.doffsets.as<uint64_t>(), iv.n,
                    stream, &iv.ndirect))
  {
    return -100;
  }
  return 0;
}

// T2: uncut patterns -- straight to the output, suffix array order
template <typename IDX>
int apm_direct(const DevIndex<IDX> &ix, const DevQueries &qs,
               const uint32_t *dk, int words, bool doedist,
               TreeIntervals &iv, hipStream_t stream, DevBuf &directm)
{
  const uint64_t ndirect = iv.ndirect;
  DevBuf hitpos, hitregion, rq, rlo, rhi;
  if (directm.alloc(ndirect * sizeof(vsa_match)) ||
      (doedist && (hitpos.alloc(ndirect * sizeof(IDX)) ||
                   hitregion.alloc(ndirect * 4) || rq.alloc(ndirect * 4) ||
                   rlo.alloc(ndirect * sizeof(IDX)) ||
                   rhi.alloc(ndirect * sizeof(IDX)))))
  {
    return -100;
  }
  k_apm_directhits<IDX, IDX><<<gridfor(ndirect), VSA_BLOCK, 0, stream>>>(
      ix, qs, dk, iv.n, iv.left.as<uint64_t>(), iv.doffsets.as<uint64_t>(),
      iv.value.as<uint32_t>(), iv.query.as<uint32_t>(), ndirect, doedist,
      directm.as<vsa_match>(), hitpos.as<IDX>(), hitregion.as<uint32_t>(),
      rq.as<uint32_t>(), rlo.as<IDX>(), rhi.as<IDX>());
  VSA_HIP(hipGetLastError());
  return doedist ? apm_longest<IDX>(ix.tis, qs, dk, words, ndirect,
                                    hitpos.as<IDX>(),
                                    hitregion.as<uint32_t>(),
                                    rq.as<uint32_t>(), rlo.as<IDX>(),
                                    rhi.as<IDX>(), directm.as<vsa_match>(),
                                    stream)
                 : 0;
}

// T4: one list in query order (merged) from the two; both are in that order
// already, and every query is answered by one of them
static int apm_mergelists(const DevQueries &qs, uint64_t nq, DevBuf &splitm,
                          uint64_t nsplit, DevBuf &directm, uint64_t ndirect,
                          hipStream_t stream, DevBuf &merged)
{
  const uint64_t nhits = nsplit + ndirect;
  DevBuf all, qkeys, qkeys2, qindex, qindex2, temp;
  if (nsplit == 0 || ndirect == 0)
  {
    merged.p = nsplit != 0 ? splitm.release() : directm.release();
    return 0;
  }
  if (all.alloc(nhits * sizeof(vsa_match)) || qkeys.alloc(nhits * 4) ||
      qkeys2.alloc(nhits * 4) || qindex.alloc(nhits * 4) ||
      qindex2.alloc(nhits * 4) || merged.alloc(nhits * sizeof(vsa_match)))
  {
    return -100;
  }
  VSA_HIP(hipMemcpyAsync(all.p, splitm.p, nsplit * sizeof(vsa_match),
                         hipMemcpyDeviceToDevice, stream));
  VSA_HIP(hipMemcpyAsync(all.as<vsa_match>() + nsplit, directm.p,
                         ndirect * sizeof(vsa_match),
                         hipMemcpyDeviceToDevice, stream));
  k_apm_querykeys<<<gridfor(nhits), VSA_BLOCK, 0, stream>>>(
      all.as<vsa_match>(), nhits, qs.seqoffset, qkeys.as<uint32_t>(),
      qindex.as<uint32_t>());
  VSA_HIP(hipGetLastError());
  VSA_HIP(rocprim_run(temp, [&](void *p, size_t &tb) {
    return rocprim::radix_sort_pairs(
        p, tb, qkeys.as<uint32_t>(), qkeys2.as<uint32_t>(),
        qindex.as<uint32_t>(), qindex2.as<uint32_t>(), (size_t) nhits, 0u,
        bitsfor(nq), stream);
  }));
  k_apm_gathermatches<<<gridfor(nhits), VSA_BLOCK, 0, stream>>>(
      all.as<vsa_match>(), qindex2.as<uint32_t>(), nhits,
      merged.as<vsa_match>());
  VSA_HIP(hipGetLastError());
  return 0;
}

template <typename IDX>
int run_approx_tree(const vsa_index *index, const vsa_queries *queries,
                    bool doedist, const TreePlan &plan, vsa_result *res)
{
  hipStream_t stream = index->stream;
  vsa_dev_set_stream(stream);
  Timer tall(stream), tsearch(stream);
  const DevIndex<IDX> ix = index->view<IDX>();
  const DevQueries qs = devqueries(queries);
  const uint64_t nq = plan.qlimit, npieces = plan.piecebase[nq];
  const int words = (int) ((plan.maxm + 63) / 64);
  ApmPieces pc;
  TreeIntervals iv;
  ApmRegions rg;
  DevBuf splitm, directm, merged;
  uint64_t nsplit = 0;
  int rc;

  res->stats.searches = npieces;
  if (nq == 0 || npieces == 0)
  {
    return 0;
  }
  if ((rc = apm_positionbits<IDX>(index, queries, 0x7FFFFFFFull,
                                  &rg.pbits)) != 0)
  {
    return rc;
  }
  if (pc.alloc(nq, npieces) || iv.alloc(nq, npieces))
  {
    return -100;
  }
  tall.start();
  if (pc.upload(plan.k, plan.splitlen, plan.piecebase, nq, stream) ||
      pc.cut(qs, nq, stream))
  {
    return -100;
  }
  if ((rc = apm_treesearch<IDX>(ix, qs, pc, plan.mode, nq, npieces, doedist,
                                tsearch, stream, iv)) != 0)
  {
    return rc;
  }
  res->stats.candidates = iv.total + iv.ndirect;
  if (iv.total >= 0xFFFFFFFFull || iv.ndirect >= 0xFFFFFFFFull)
  {
    VSA_ERROR("approximate search: more than 2^32 piece hits");
    return -5;
  }
  if (iv.ndirect > 0 &&
      (rc = apm_direct<IDX>(ix, qs, pc.k.as<uint32_t>(), words, doedist, iv,
                            stream, directm)) != 0)
  {
    return rc;
  }
  // T3: pieces -- regions, merged, verified from right to left: the stages
  // of run_approx with the intervals in the place of the pieces
  if (iv.total > 0)
  {
    const ApmHits hits = {iv.left.as<uint64_t>(), iv.poffsets.as<uint64_t>(),
                          iv.query.as<uint32_t>(), iv.poffset.as<uint32_t>(),
                          iv.n, iv.total};
    if ((rc = apm_regions<IDX>(ix, qs, nq, hits, pc.k.as<uint32_t>(), doedist,
                               nullptr, stream, rg)) != 0 ||
        (rc = apm_verify<IDX>(ix.tis, qs, pc.k.as<uint32_t>(), words, doedist,
                              rg, stream, splitm, &nsplit)) != 0)
    {
      return rc;
    }
  }
  if (apm_mergelists(qs, nq, splitm, nsplit, directm, iv.ndirect, stream,
                     merged))
  {
    return -100;
  }
  return finish(res, merged, nsplit + iv.ndirect, tall, tsearch, stream);
}
