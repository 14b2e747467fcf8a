// The walk of the planned MUM search: one lane, one chunk of a plan range --
// included by mum_workplan.inc in front of k_query_search_planned, which has
// the reasoning and the layout of the chunks, and k_mum_walk_tiles, which
// hands the chunks out.
//
// Offsets [first, off] of read q, located from `off` down.  After the locate
// of offset h with U, an upper bound of the longest match there, the lane
// goes on at min(h - 1, h + U - searchlength): the offsets between cannot
// reach searchlength symbols (e(j) <= e(h) for j < h).  Every located offset
// takes the candidate test and the output form of k_query_search<IDX, MUM>.
//
// vsa_walk_step is one trip of a wavefront through that: the locate of `off`,
// the candidate test, the append, the bound and the next offset.  All lanes of
// a wavefront call it together (the deep locate wants them all), lanes without
// an offset pass active = false.  It adds the lane's locate to `locates` and
// leaves `off` at the next offset to locate, `active` false once the chunk is
// done.  Both loops of the planned search go through it: vsa_walk_chunk below
// (a lane keeps its chunk until the wavefront is done) and the tile queue of
// k_mum_walk_tiles (free lanes take new chunks between two steps).
// PQ: the read through windows of its packed row *rq (no special symbol in
// it); else through `read`, its bytes (a pointer, or the QSrc of a read of a
// packed batch that has a special symbol: the same locate, the same bounds and
// so the same walk as in the byte batch of the same reads).
template <typename IDX, bool DEEP, bool PQ, typename QP>
__device__ __forceinline__ void
vsa_walk_step(const DevIndex<IDX> &ix, const DevQueries &qs, bool &active,
              QP read, const RowQuery *rq, uint32_t qlen, uint32_t first,
              uint32_t &off, uint64_t q, const uint64_t *__restrict__ base,
              uint32_t perquery, uint32_t searchlength,
              vsa_match *__restrict__ out, uint64_t *__restrict__ outkey,
              uint64_t shardcap, uint32_t shard,
              unsigned long long *__restrict__ cursors, uint32_t packbits,
              uint32_t valbits, uint32_t &locates)
{
  uint32_t c = 0, maxlcp = 0;
  uint64_t witness = 0;
  uint8_t leftchar = (uint8_t) VSA_SEPARATOR;
  const uint32_t remaining = qlen - off;
  const QP qptr = read + off;
  bool have = false, fast = false;
  DeepHit hit;
  int st = VSA_LOC_SLOW;
  locates += active ? 1u : 0u;
  if (active && off > 0)
  {
    if constexpr (PQ)
    {
      leftchar = (uint8_t) (vsa_pq_window(*rq, off - 1) >> 62);
    } else
    {
      leftchar = vsa_qsym(read, off - 1);
    }
  }
  if constexpr (DEEP)
  {
    const uint32_t qleft = off > 0 ? (uint32_t) leftchar : 0x100u;
    if constexpr (PQ)
    {
      // windows of the row (one 16-byte load each)
      st = vsa_locate_deep<1, true>(ix, active, qptr, remaining, maxlcp,
                                    witness, hit, searchlength, qleft, rq,
                                    off);
    } else
    {
      st = vsa_locate_deep(ix, active, qptr, remaining, maxlcp, witness,
                           hit, searchlength, qleft);
    }
  }
  if (st == VSA_LOC_SLOW)
  {
    have = active &&
           vsa_locate_reference(ix, qptr, remaining, maxlcp, witness);
  } else
  {
    have = st == VSA_LOC_FOUND;
    fast = have && maxlcp < 255;
  }
  // (a work-item none of whose matches can be left maximal was cut short
  // by the locate: hit.notleftmax, maxlcp is only a lower bound then)
  const bool cutshort = st != VSA_LOC_SLOW && hit.notleftmax;
  if (have && maxlcp >= searchlength && !cutshort)
  {
    if (fast)
    {
      // leftrightmaximaluniquematch (fquery.c:297-386) and PROCESSSUFFIX
      // (fquery.c:54-81) on values already in registers
      // (suffix 0 has the separator of the front pad as hit.leftsym)
      const uint32_t lcpw = (uint32_t) (hit.ew >> 32) & 0xFFu;
      const bool unique = (witness == 0 || lcpw < maxlcp) &&
                          (witness + 1 > ix.n - 1 || hit.lcpnext < maxlcp);
      c = (unique && (VSA_ISSPECIAL(leftchar) || leftchar != hit.leftsym))
              ? 1u
              : 0u;
    } else
    {
      c = (vsa_mum_candidate<IDX, DEEP>(ix, maxlcp, witness) &&
           vsa_leftmaximal(ix, vsa_sufstart<IDX, DEEP>(ix, witness),
                           leftchar))
              ? 1u
              : 0u;
    }
  }
  const uint64_t inshard = vsa_wave_reserve01(
      cursors + (uint64_t) shard * VSA_CURSOR_STRIDE, c != 0);
  if (c != 0 && inshard < shardcap)
  {
    const uint64_t dbstart = fast ? vsa_entrystart(ix, hit.ew, witness)
                                  : vsa_sufstart<IDX, DEEP>(ix, witness);
    const uint64_t t0 = (base != nullptr) ? base[q] : q * perquery;
    vsa_write_candidate(qs, out, outkey,
                        (uint64_t) shard * shardcap + inshard, q, off,
                        t0 + off, dbstart, maxlcp, packbits, valbits);
  }
  if (active)
  {
    // U: exact from the reference walk and from a deep locate that ran to
    // its end; fewer than prefixlength (no bucket) or D (no deep bucket)
    // symbols otherwise; none after a locate that was cut short
    uint32_t bound;
    if (st == VSA_LOC_SLOW)
    {
      bound = have ? maxlcp : ix.pl - 1;
    } else
    {
      bound = have ? maxlcp : ix.D - 1;
    }
    const uint32_t reach = off + bound; // e(off) at most
    uint32_t next = off - 1;            // (off = 0: the walk ends below)
    bool left = off > first;
    if (!cutshort && reach + 1 < off + searchlength)
    {
      left = left && reach >= searchlength;
      next = reach - searchlength;
    }
    active = left && next >= first;
    off = next;
  }
}

// one lane, one chunk: the loop leaves when no lane of the wavefront has an
// offset left.  Returns the locates this lane made.
template <typename IDX, bool DEEP, bool PQ, typename QP>
__device__ __forceinline__ uint32_t
vsa_walk_chunk(const DevIndex<IDX> &ix, const DevQueries &qs, bool active,
               QP read, const RowQuery *rq, uint32_t qlen, uint32_t first,
               uint32_t off, uint64_t q, const uint64_t *__restrict__ base,
               uint32_t perquery, uint32_t searchlength,
               vsa_match *__restrict__ out, uint64_t *__restrict__ outkey,
               uint64_t shardcap, uint32_t shard,
               unsigned long long *__restrict__ cursors, uint32_t packbits,
               uint32_t valbits)
{
  uint32_t locates = 0;
  while (__any(active))
  {
    vsa_walk_step<IDX, DEEP, PQ>(ix, qs, active, read, rq, qlen, first, off, q,
                                 base, perquery, searchlength, out, outkey,
                                 shardcap, shard, cursors, packbits, valbits,
                                 locates);
  }
  return locates;
}
