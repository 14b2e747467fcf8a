// vmatch -pp matchcluster erate E on the device: the edge source of
// matchcluster.hip for the handles of vsa_eratecluster_open.  Included
// by matchcluster.hip inside its unnamed namespace; the rules are
// erate_rules.h, the same text the host compiles.
//
//   refs     k_er_refs, one lane per record of a list: the view of a self
//            list, vsa_er_checkplace, and a look for separators eight
//            symbols per load (a record that leaves the text or holds a
//            separator does not fit).
//   rows     the window of match i is every j > i: count_i = n - 1 - i,
//            scanned into the row offsets off_i that k_mc_tilefirst and
//            mc_owner already search.  At most VSA_MATCHCLUSTER_CHUNK slots
//            per pass; everything below is per pass.
//   length   LenF, one lane per slot: the length test.  The pairs that pass
//            are compacted (tile_compact.inc, stable: slot order) into
//            (i, j); a pair whose bound is above VSA_ERATE_MAXDIST is counted
//            and ends the finish.
//   widths   WidthF, one lane per surviving pair: the class of its bound
//            (2 * maxdist + 1 diagonals on 16, 32 or 64 lanes, or 2 or 4
//            diagonals on each of 64 lanes), compacted into one list of
//            survivor numbers per class.
//   distance k_er_dist<W, D, ROW>, one group of W lanes per surviving pair,
//            the lanes are the diagonals of the greedy front: lane l holds
//            the D diagonals l * D + q - maxdist in registers, as 32-bit rows
//            while every match of the list is shorter than 2^30 symbols
//            (VSA_ERATE_WIDE_ROWS in the environment asks for the 64-bit
//            rows of longer lists anyway).  Every trip of the
//            loop is one round of one instance pair: the neighbours' rows by
//            shuffles inside the group, vsa_er_best, the slide along the
//            text eight symbols per load, and a ballot for the goal.  The
//            groups of a wavefront walk their cascades independently, the
//            loop ends when the last one is through.  answer[s] = the
//            distance of the first instance pair within the bound, or -1.
//   edges    EdgeF, one lane per surviving pair: those with an answer go
//            through the same compaction behind the edges so far.
// Survivor numbers are 32 bit: a pass has at most 2^31 slots.

#define ER_BLOCK 256
#define ER_WIDTHS 5
#define ER_MAXCHUNK ((uint64_t) 1 << 31)

static_assert(VSA_ERATE_MAXDIST == 127,
              "the widest class holds 64 * 4 >= 2 * VSA_ERATE_MAXDIST + 1 "
              "diagonals");

// the class of a bound <= VSA_ERATE_MAXDIST: (W, D) = (16, 1), (32, 1),
// (64, 1), (64, 2), (64, 4); W * D >= 2 * maxdist + 1
__host__ __device__ inline int er_widthclass(uint64_t maxdist)
{
  return maxdist <= 7 ? 0 : maxdist <= 15 ? 1 : maxdist <= 31 ? 2
         : maxdist <= 63 ? 3 : 4;
}

// ---- refs -----------------------------------------------------------------------

// a separator among text[p .. p + length): eight symbols per load while eight
// are left, so nothing behind the instance is read.  A byte is 255 iff its
// complement is 0; the zero-byte test is exact for "any".
__device__ __forceinline__ bool er_hasseparator(const uint8_t *__restrict__ p,
                                                uint64_t length)
{
  uint64_t x = 0;
  for (; x + 8 <= length; x += 8)
  {
    const uint64_t v = ~vsa_load8(p + x);
    if (((v - 0x0101010101010101ull) & ~v & 0x8080808080808080ull) != 0)
    {
      return true;
    }
  }
  for (; x < length; x++)
  {
    if (p[x] == VSA_SEPARATOR)
    {
      return true;
    }
  }
  return false;
}

// One lane per record; a lane reads its two instances alone, 2 * length
// bytes of text against the 32 of its record.  Lists of this step are short
// (the pairs are quadratic) and the stage stays below a millisecond at 10^4
// matches of 1000 symbols, so the instances are not spread over lanes.
// bad[0]: records that do not fit, bad[1]: records of 2^32 symbols or more,
// bad[2]: the longest length of the others
__global__ void __launch_bounds__(TC_BLOCK)
k_er_refs(vsa_selrules view, const uint8_t *__restrict__ text,
          uint64_t textlength, const vsa_match *__restrict__ in, uint64_t n,
          uint64_t base, vsa_match *__restrict__ recs,
          uint8_t *__restrict__ flags, uint64_t *__restrict__ start,
          uint64_t *__restrict__ length, unsigned long long *__restrict__ bad)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  int rc = 0;
  if (i < n)
  {
    const vsa_match m = in[i];
    vsa_selvalues v;
    rc = vsa_sel_values(&view, &m, 0, &v) != 0 ? -2 : 0;
    if (rc == 0)
    {
      rc = vsa_er_checkplace(textlength, v.length1, v.position1, v.position2);
    }
    if (rc == 0 && (er_hasseparator(text + v.position1, v.length1) ||
                    er_hasseparator(text + v.position2, v.length1)))
    {
      rc = -2;
    }
    if (rc == 0)
    {
      atomicMax(&bad[2], (unsigned long long) v.length1);
      const uint64_t at = base + i;
      recs[at] = m;
      flags[at] = 0;
      start[2 * at] = v.position1;
      start[2 * at + 1] = v.position2;
      length[at] = v.length1;
    }
    else if (rc != -2)
    {
      atomicAdd(&bad[1], 1ull);
    }
  }
  wave_count(rc == -2, &bad[0]);
}

// ---- rows -----------------------------------------------------------------------

// count[i] = the matches behind match i; count[n] = 0 for the scan
__global__ void __launch_bounds__(TC_BLOCK)
k_er_rows(uint64_t n, uint64_t *__restrict__ count)
{
  const uint64_t i = vsa_bid() * TC_BLOCK + threadIdx.x;
  if (i <= n)
  {
    count[i] = i < n ? n - 1 - i : 0;
  }
}

// ---- length ---------------------------------------------------------------------

struct ErPair
{
  uint32_t i, j;
};

struct LenF
{
  typedef ErPair Payload;
  const uint64_t *off, *first, *length;
  uint64_t c0; // slots of the passes before
  uint32_t errorrate;
  uint32_t *si, *sj;

  __device__ int cls(uint64_t k, Payload &p) const
  {
    const uint64_t s = c0 + k, t = k / TC_TILE;
    const uint64_t i = mc_owner(off, first[t], first[t + 1], s);
    const uint64_t j = i + 1 + (s - off[i]);
    const uint64_t li = length[i], lj = length[j];
    const uint64_t maxdist = vsa_er_maxdist(li < lj ? li : lj, errorrate);
    p.i = (uint32_t) i;
    p.j = (uint32_t) j;
    if (vsa_er_lengthfails(li, lj, maxdist))
    {
      return VSA_ER_LENGTH;
    }
    return maxdist > VSA_ERATE_MAXDIST ? VSA_ER_TOOFAR : VSA_ER_SURVIVOR;
  }
  __device__ void put(int, uint64_t rank, uint64_t, const Payload &p) const
  {
    si[rank] = p.i;
    sj[rank] = p.j;
  }
};

// ---- widths ---------------------------------------------------------------------

struct WidthF
{
  typedef NoPayload Payload;
  const uint64_t *length;
  const uint32_t *si, *sj;
  uint32_t errorrate;
  uint64_t classbase[ER_WIDTHS];
  uint32_t *order;

  __device__ int cls(uint64_t s, Payload &) const
  {
    const uint64_t li = length[si[s]], lj = length[sj[s]];
    return er_widthclass(vsa_er_maxdist(li < lj ? li : lj, errorrate));
  }
  __device__ void put(int q, uint64_t rank, uint64_t s, const Payload &) const
  {
    order[classbase[q] + rank] = (uint32_t) s;
  }
};

// ---- distance -------------------------------------------------------------------

// vsa_er_slide, eight symbols per load where eight are left on both sides:
// nothing is read behind an instance, and so nothing outside the text
__device__ __forceinline__ int64_t er_slide(const uint8_t *__restrict__ text,
                                            uint64_t pu, uint64_t ulen,
                                            uint64_t pv, uint64_t vlen,
                                            int64_t t, int64_t k)
{
  const int64_t ru = (int64_t) ulen - t, rv = (int64_t) vlen - (t + k);
  const int64_t rem = ru < rv ? ru : rv;
  const uint8_t *a = text + pu + (uint64_t) t,
                *b = text + pv + (uint64_t) (t + k);
  int64_t x = 0;
  while (x + 8 <= rem)
  {
    const uint64_t wa = vsa_load8(a + x), wb = vsa_load8(b + x);
    const uint64_t m = (wa ^ wb) | vsa_specialmask(wa);
    if (m != 0)
    {
      return t + x + (int64_t) (__builtin_ctzll(m) >> 3);
    }
    x += 8;
  }
  while (x < rem && vsa_er_symequal(a[x], b[x]))
  {
    x++;
  }
  return t + x;
}

// The rows of a front are ROW words: int32_t while every length of the list
// is below ER_NARROW (a row is at most a length plus one) -- one shuffle per
// neighbour and half the registers --, else int64_t.  ErNeg<ROW> is "no row":
// below every row, and still below 0 after VSA_ERATE_MAXDIST increments.
#define ER_NARROW ((uint64_t) 1 << 30)

template <typename ROW>
struct ErNeg;
template <>
struct ErNeg<int32_t>
{
  static constexpr int32_t value = -((int32_t) 1 << 30);
};
template <>
struct ErNeg<int64_t>
{
  static constexpr int64_t value = VSA_ER_NEG;
};

__device__ __forceinline__ int32_t er_shfl_up(int32_t v, int width)
{
  return __shfl_up(v, 1, width);
}

__device__ __forceinline__ int32_t er_shfl_down(int32_t v, int width)
{
  return __shfl_down(v, 1, width);
}

__device__ __forceinline__ int64_t er_shfl_up(int64_t v, int width)
{
  const int lo = __shfl_up((int) (uint32_t) (uint64_t) v, 1, width),
            hi = __shfl_up((int) (uint32_t) ((uint64_t) v >> 32), 1, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

__device__ __forceinline__ int64_t er_shfl_down(int64_t v, int width)
{
  const int lo = __shfl_down((int) (uint32_t) (uint64_t) v, 1, width),
            hi = __shfl_down((int) (uint32_t) ((uint64_t) v >> 32), 1, width);
  return (int64_t) ((uint64_t) (uint32_t) hi << 32 | (uint32_t) lo);
}

template <int W, int D, typename ROW>
__global__ void __launch_bounds__(ER_BLOCK)
k_er_dist(const uint8_t *__restrict__ text, const uint64_t *__restrict__ start,
          const uint64_t *__restrict__ length, const uint32_t *__restrict__ si,
          const uint32_t *__restrict__ sj, const uint32_t *__restrict__ order,
          uint64_t count, uint32_t errorrate, int32_t *__restrict__ answer)
{
  static_assert(W == 16 || W == 32 || W == 64, "a group divides a wavefront");
  const uint64_t g = (vsa_bid() * ER_BLOCK + threadIdx.x) / W;
  const int gl = (int) (threadIdx.x % W);
  bool active = g < count;
  uint32_t s = 0;
  uint64_t ulen = 0, vlen = 0, maxdist = 0, pu = 0, pv = 0;
  uint64_t pi[2] = {0, 0}, pj[2] = {0, 0};
  if (active)
  {
    s = order[g];
    const uint32_t i = si[s], j = sj[s];
    ulen = length[i];
    vlen = length[j];
    maxdist = vsa_er_maxdist(ulen < vlen ? ulen : vlen, errorrate);
    pi[0] = start[2 * (uint64_t) i];
    pi[1] = start[2 * (uint64_t) i + 1];
    pj[0] = start[2 * (uint64_t) j];
    pj[1] = start[2 * (uint64_t) j + 1];
  }
  const int64_t goal = (int64_t) vlen - (int64_t) ulen,
                k0 = (int64_t) gl * D - (int64_t) maxdist;
  // the bits of this group in a ballot
  const uint32_t shift = (threadIdx.x & 63u) & ~(uint32_t) (W - 1);
  const uint64_t groupbits = W == 64 ? ~(uint64_t) 0
                                     : (((uint64_t) 1 << (W & 63)) - 1);
  constexpr ROW NEG = ErNeg<ROW>::value;
  ROW t[D];
#pragma unroll
  for (int q = 0; q < D; q++)
  {
    t[q] = NEG;
  }
  int c = 0, answered = -1;
  uint64_t d = 0;
  while (__ballot(active) != 0)
  {
    // (all lanes: the rows of the neighbouring diagonals in other lanes)
    ROW below = er_shfl_up(t[D - 1], W), above = er_shfl_down(t[0], W);
    if (gl == 0)
    {
      below = NEG;
    }
    if (gl == W - 1)
    {
      above = NEG;
    }
    bool atgoal = false;
    if (active)
    {
      if (d == 0)
      {
        pu = pi[vsa_er_first(c)];
        pv = pj[vsa_er_second(c)];
#pragma unroll
        for (int q = 0; q < D; q++)
        {
          t[q] = NEG;
        }
        if (vsa_er_sameinstance(pu, ulen, pv, vlen))
        {
          atgoal = true;
        } else
        {
#pragma unroll
          for (int q = 0; q < D; q++)
          {
            if (k0 + q == 0)
            {
              t[q] = (ROW) er_slide(text, pu, ulen, pv, vlen, 0, 0);
              atgoal = goal == 0 && t[q] == (int64_t) ulen;
            }
          }
        }
      } else
      {
        ROW old[D];
#pragma unroll
        for (int q = 0; q < D; q++)
        {
          old[q] = t[q];
        }
#pragma unroll
        for (int q = 0; q < D; q++)
        {
          const int64_t k = k0 + q;
          // (the neighbours inside this lane, or those of the lanes beside
          // it; the clamps keep every constant index inside old[])
          const int64_t lower = q > 0 ? old[q > 0 ? q - 1 : 0] : below,
                        upper = q < D - 1 ? old[q < D - 1 ? q + 1 : q] : above;
          int64_t r = vsa_er_best(old[q], lower, upper);
          if (r < 0 || r + k < 0)
          {
            r = VSA_ER_NEG;
          } else
          {
            r = vsa_er_sametext(pu, ulen, pv, vlen, k)
                    ? (int64_t) ulen - 1
                    : er_slide(text, pu, ulen, pv, vlen, r, k);
            r = vsa_er_stored(r, k, ulen, vlen);
          }
          t[q] = r < 0 ? NEG : (ROW) r;
          atgoal = atgoal || (k == goal && r == (int64_t) ulen);
        }
      }
    }
    const bool found = ((__ballot(atgoal) >> shift) & groupbits) != 0;
    if (active)
    {
      if (found)
      {
        answered = (int) d;
        active = false;
      } else if (d == maxdist)
      {
        // this instance pair is not within the bound: the next one
        d = 0;
        c++;
        active = c < 4;
      } else
      {
        d++;
      }
    }
  }
  if (g < count && gl == 0)
  {
    answer[s] = answered;
  }
}

template <int W, int D, typename ROW>
int er_launch(const vsa_matchcluster *c, const uint32_t *si,
              const uint32_t *sj, const uint32_t *order, uint64_t count,
              int32_t *answer)
{
  if (count == 0)
  {
    return 0;
  }
  const uint64_t groups = ER_BLOCK / W;
  k_er_dist<W, D, ROW><<<vsa_grid((count + groups - 1) / groups), ER_BLOCK, 0,
                         nullptr>>>(c->text, c->start, c->length, si, sj,
                                    order, count, c->errorrate, answer);
  VSA_HIP(hipGetLastError());
  return 0;
}

// 64-bit rows are asked for whatever the lengths are
bool widerows()
{
  const char *s = getenv("VSA_ERATE_WIDE_ROWS");
  return s != nullptr && *s != '\0' && *s != '0';
}

// the five classes of one pass; first[q] .. first[q + 1]: the places of
// class q in order[]
template <typename ROW>
int er_distances(const vsa_matchcluster *c, const uint32_t *si,
                 const uint32_t *sj, const uint32_t *order,
                 const uint64_t *first, int32_t *answer)
{
  const uint64_t *f = first;
  return er_launch<16, 1, ROW>(c, si, sj, order + f[0], f[1] - f[0],
                               answer) != 0 ||
                 er_launch<32, 1, ROW>(c, si, sj, order + f[1], f[2] - f[1],
                                       answer) != 0 ||
                 er_launch<64, 1, ROW>(c, si, sj, order + f[2], f[3] - f[2],
                                       answer) != 0 ||
                 er_launch<64, 2, ROW>(c, si, sj, order + f[3], f[4] - f[3],
                                       answer) != 0 ||
                 er_launch<64, 4, ROW>(c, si, sj, order + f[4], f[5] - f[4],
                                       answer) != 0
             ? -100
             : 0;
}

// ---- edges ----------------------------------------------------------------------

struct EdgeF
{
  typedef PairPayload Payload;
  const uint64_t *length;
  const uint32_t *si, *sj;
  const int32_t *answer;
  uint64_t base; // edges of the passes before
  uint32_t *e1, *e2;
  uint64_t *value;

  __device__ int cls(uint64_t s, Payload &p) const
  {
    const int32_t a = answer[s];
    if (a < 0)
    {
      return 1;
    }
    p.mi = si[s];
    p.mj = sj[s];
    const uint64_t li = length[p.mi], lj = length[p.mj];
    p.value = vsa_er_value(li < lj ? li : lj, (uint64_t) a);
    return 0;
  }
  __device__ void put(int, uint64_t rank, uint64_t, const Payload &p) const
  {
    e1[base + rank] = p.mi;
    e2[base + rank] = p.mj;
    value[base + rank] = p.value;
  }
};

// ---- host -----------------------------------------------------------------------

// rows, length, widths, distance, edges: the edges of the n >= 2 matches into
// `edges`; st->candidates and below are counted
int findedges_erate(vsa_matchcluster *c, EdgeList &edges,
                    vsa_matchclusterstats *st, double *ms)
{
  const uint64_t n = c->list.n;
  const uint32_t E = c->errorrate;
  DevBuf count, off;
  Timer trows(nullptr), tpairs(nullptr);
  if (count.alloc((n + 1) * 8) != 0 || off.alloc((n + 1) * 8) != 0)
  {
    return -100;
  }
  trows.start();
  k_er_rows<<<gridfor(n + 1), TC_BLOCK, 0, nullptr>>>(n,
                                                       count.as<uint64_t>());
  VSA_HIP(hipGetLastError());
  uint64_t total = 0;
  if (exclusive_sum(count.as<uint64_t>(), off.as<uint64_t>(), n, nullptr,
                    &total) != 0)
  {
    return -100;
  }
  trows.stop();
  st->candidates = total;
  tpairs.start();
  const uint64_t chunk = std::min<uint64_t>(chunkslots(), ER_MAXCHUNK);
  for (uint64_t c0 = 0; c0 < total; c0 += chunk)
  {
    const uint64_t ns = std::min<uint64_t>(chunk, total - c0),
                   nt = tilesof(ns);
    DevBuf first, offsets, si, sj, order, answer;
    uint64_t totals[VSA_ER_CLASSES];
    if (first.alloc((nt + 1) * 8) != 0)
    {
      return -100;
    }
    k_mc_tilefirst<<<gridfor(nt + 1), TC_BLOCK, 0, nullptr>>>(
        off.as<uint64_t>(), n, c0, ns, nt, first.as<uint64_t>());
    VSA_HIP(hipGetLastError());
    LenF lf;
    lf.off = off.as<uint64_t>();
    lf.first = first.as<uint64_t>();
    lf.length = c->length;
    lf.c0 = c0;
    lf.errorrate = E;
    lf.si = lf.sj = nullptr;
    if (tc_count<1, VSA_ER_CLASSES>(lf, ns, offsets, totals) != 0)
    {
      return -100;
    }
    if (totals[VSA_ER_TOOFAR] != 0)
    {
      VSA_ERROR("vsa_matchcluster_finish: %lu pairs pass the length test with "
                "a bound above %d edit operations: vsa_eratecluster_host "
                "takes such lists", (unsigned long) totals[VSA_ER_TOOFAR],
                VSA_ERATE_MAXDIST);
      return VSA_NOT_COVERED;
    }
    const uint64_t nsurv = totals[VSA_ER_SURVIVOR];
    if (nsurv > 0)
    {
      if (si.alloc(nsurv * 4) != 0 || sj.alloc(nsurv * 4) != 0 ||
          order.alloc(nsurv * 4) != 0 || answer.alloc(nsurv * 4) != 0)
      {
        return -100;
      }
      lf.si = si.as<uint32_t>();
      lf.sj = sj.as<uint32_t>();
      if (tc_emit<1>(lf, ns, offsets) != 0)
      {
        return -100;
      }
      // the survivors by the width of their front
      WidthF wf;
      wf.length = c->length;
      wf.si = si.as<uint32_t>();
      wf.sj = sj.as<uint32_t>();
      wf.errorrate = E;
      wf.order = order.as<uint32_t>();
      DevBuf woffsets;
      uint64_t wtotals[ER_WIDTHS], wbase[ER_WIDTHS + 1];
      if (tc_count<ER_WIDTHS, ER_WIDTHS>(wf, nsurv, woffsets, wtotals) != 0)
      {
        return -100;
      }
      wbase[0] = 0;
      for (int q = 0; q < ER_WIDTHS; q++)
      {
        wf.classbase[q] = wbase[q];
        wbase[q + 1] = wbase[q] + wtotals[q];
      }
      if (tc_emit<ER_WIDTHS>(wf, nsurv, woffsets) != 0)
      {
        return -100;
      }
      const uint32_t *o = order.as<uint32_t>();
      int32_t *ans = answer.as<int32_t>();
      if ((c->longest < ER_NARROW && !widerows()
               ? er_distances<int32_t>(c, wf.si, wf.sj, o, wbase, ans)
               : er_distances<int64_t>(c, wf.si, wf.sj, o, wbase, ans)) != 0)
      {
        return -100;
      }
      EdgeF ef;
      ef.length = c->length;
      ef.si = wf.si;
      ef.sj = wf.sj;
      ef.answer = ans;
      ef.base = edges.list.n;
      ef.e1 = ef.e2 = nullptr;
      ef.value = nullptr;
      DevBuf eoffsets;
      uint64_t etotals[2];
      if (tc_count<1, 2>(ef, nsurv, eoffsets, etotals) != 0)
      {
        return -100;
      }
      const uint64_t m = etotals[0];
      if (edges.list.n + m >= 0xFFFFFFFFull)
      {
        VSA_ERROR("vsa_matchcluster_finish: %lu edges: only fewer than 2^32 - "
                  "1 are covered", (unsigned long) (edges.list.n + m));
        return VSA_NOT_COVERED;
      }
      if (m > 0)
      {
        if (edges.list.reserve(edges.list.n + m) != 0)
        {
          return -100;
        }
        ef.e1 = edges.e1;
        ef.e2 = edges.e2;
        ef.value = edges.value;
        if (tc_emit<1>(ef, nsurv, eoffsets) != 0)
        {
          return -100;
        }
        edges.list.n += m;
      }
    }
    // (the buffers of this pass are read by its kernels)
    VSA_HIP(hipStreamSynchronize(nullptr));
  }
  tpairs.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  st->below = total - edges.list.n;
  ms[MC_WINDOW] += trows.ms();
  ms[MC_PAIRS] += tpairs.ms();
  return 0;
}
