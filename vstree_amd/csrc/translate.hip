// vmatch -dnavsprot on the GPU (include/vstree_amd.h): the six-frame
// translation of DNA queries into an ordinary batch of protein queries, and
// the conversion of the match lists of such a batch back to DNA coordinates.
// The rules are those of sixframe_rules.h, which translate_host.c applies on
// the host; tests/test_gpu_translated.py demands the same bytes of both.
//
// The translation is a streaming kernel.  The codons of all six frames of a
// sequence lie on the three grids g = 0, 1, 2 of its forward strand
// (sixframe_rules.h: vsa_sf_reverseframe), so ONE look at the characters 3 j
// .. 3 j + 4 -- a "slot" -- gives symbol j of the three forward frames and one
// symbol of each reverse frame.  The slots of all sequences with a codon,
// numbered through, are dealt out VSA_TRANSLATE_TILE to a workgroup, one to a
// work-item: short reads share a workgroup, a long sequence is cut into
// tiles.  A work-item loads the three characters of its slot, turns them into
// 4-bit base sets and leaves them in LDS, 12 bits to a slot; the two
// characters of halo are the first two of the next slot, read back from
// there (from memory where the next slot belongs to another workgroup, and at
// the end of a sequence, whose last len mod 3 characters are in no slot).
// A codon of plain bases is one look into a 64-entry table with the symbol
// map of the index folded in; a codon with a wildcard takes the rule path.
// Consecutive work-items write consecutive symbols of a frame (descending in
// the reverse frames): every frame is written coalesced.  Measured:
// profiles/r14/README.md (the kernel moves one byte per lane and memory
// instruction and reaches 14 % of the streaming read rate).
#include <vector>
#include "vsa_internal.hpp"
#include "search_host.hpp"
#include "sixframe_rules.h"

extern "C" uint64_t vsa_translate_tile(void)
{
  return VSA_TRANSLATE_TILE;
}

extern "C" double vsa_queries_translate_ms(const vsa_queries *q)
{
  return q == nullptr ? 0.0 : q->translate_ms;
}

namespace
{

#define SF_ERR_UNMAPPED 1u // an amino acid outside the alphabet
#define SF_ERR_ILLEGAL 2u  // a character the translation does not know

// what the kernel reads besides the characters: the base set of every
// character (vsa_sf_class as a table: as a switch every lane of a wavefront
// walks its own branch), the 64 letters of the translation table, the same
// through the symbol map, the symbol map
struct SfTables
{
  uint8_t cls[256];
  uint8_t aminos[64];
  uint8_t mapped[64];
  uint8_t symbolmap[256];
  uint32_t numofchars;
};

// the sequences that have a codon, in order ("compact"): where their
// characters start, how many there are, where frame 0 goes; cslot[c] = the
// number of slots in front of sequence c (one entry more: the total);
// blockfirst[b] = the compact sequence the first slot of workgroup b lies in
// (one entry more).  UNIFORM: every sequence has m characters, sequence s
// starts at s * m and its frame 0 at s * span: no tables.
struct SfLayout
{
  const uint64_t *cstart, *clen, *cpbase, *cslot;
  const uint32_t *blockfirst;
  uint64_t nslots;
  uint64_t m, span, slotsper, nsymbols; // UNIFORM
};

__device__ __forceinline__ uint32_t sf_classof(const SfTables *t,
                                               const uint8_t *chars,
                                               uint64_t pos, uint64_t len,
                                               uint64_t at, uint32_t *err)
{
  // (at < len is the caller's)
  const uint32_t cls = t->cls[chars[pos + at]];
  if (vsa_sf_illegal(len, cls))
  {
    *err = SF_ERR_ILLEGAL;
  }
  return cls;
}

template <bool UNIFORM>
__global__ void __launch_bounds__(VSA_TRANSLATE_TILE)
k_sf_translate(const uint8_t *__restrict__ chars, const SfLayout lay,
               const SfTables *__restrict__ tables,
               uint8_t *__restrict__ protein, uint32_t *__restrict__ errflag)
{
  __shared__ SfTables t;
  __shared__ uint16_t slotcls[VSA_TRANSLATE_TILE];
  // (the sequences of its slots, that of the next workgroup's first slot, and
  // the entry behind them)
  __shared__ uint64_t seqslot[UNIFORM ? 1 : VSA_TRANSLATE_TILE + 2];
  const uint32_t i = threadIdx.x;
  const uint64_t v0 = vsa_bid() * VSA_TRANSLATE_TILE, v = v0 + i;
  uint32_t nseq = 0;
  uint64_t cfirst = 0;

  if (i < sizeof(SfTables) / 4)
  {
    ((uint32_t *) &t)[i] = ((const uint32_t *) tables)[i];
  }
  if (!UNIFORM && v0 < lay.nslots)
  {
    // the sequences this workgroup's slots lie in: at most one per slot
    cfirst = lay.blockfirst[vsa_bid()];
    nseq = lay.blockfirst[vsa_bid() + 1] - (uint32_t) cfirst + 1;
    for (uint32_t k = i; k <= nseq; k += VSA_TRANSLATE_TILE)
    {
      seqslot[k] = lay.cslot[cfirst + k];
    }
  }
  __syncthreads();
  const bool active = v < lay.nslots;
  uint64_t pos = 0, len = 0, pbase = 0, j = 0;
  if (active)
  {
    if (UNIFORM)
    {
      // (a 64-bit division costs tens of instructions: batches of fewer than
      // 2^32 slots, all that fit a device today, divide in 32 bits)
      if (lay.nslots <= 0xFFFFFFFFull && lay.span <= 0xFFFFFFFFull)
      {
        const uint32_t s = (uint32_t) v / (uint32_t) lay.slotsper;
        j = (uint32_t) v - s * (uint32_t) lay.slotsper;
        // (m and span are below 2^32: one multiply-add each)
        pos = (uint64_t) s * (uint32_t) lay.m;
        pbase = (uint64_t) s * (uint32_t) lay.span;
      } else
      {
        const uint64_t s = v / lay.slotsper;
        j = v - s * lay.slotsper;
        pos = s * lay.m;
        pbase = s * lay.span;
      }
      len = lay.m;
    } else
    {
      // the last sequence that starts at or before slot v
      uint32_t lo = 0, hi = nseq - 1;
      while (lo < hi)
      {
        const uint32_t mid = (lo + hi + 1) / 2;
        if (seqslot[mid] <= v)
        {
          lo = mid;
        } else
        {
          hi = mid - 1;
        }
      }
      j = v - seqslot[lo];
      pos = lay.cstart[cfirst + lo];
      len = lay.clen[cfirst + lo];
      pbase = lay.cpbase[cfirst + lo];
    }
  }
  uint32_t err = 0, k[5] = {0, 0, 0, 0, 0};
  const uint64_t nslots = len / 3u; // of this sequence
  if (active)
  {
    k[0] = sf_classof(&t, chars, pos, len, 3u * j, &err);
    k[1] = sf_classof(&t, chars, pos, len, 3u * j + 1u, &err);
    k[2] = sf_classof(&t, chars, pos, len, 3u * j + 2u, &err);
    slotcls[i] = (uint16_t) (k[0] | k[1] << 4 | k[2] << 8);
  }
  __syncthreads();
  if (active)
  {
    if (j + 1u < nslots && i + 1u < VSA_TRANSLATE_TILE)
    {
      // (slot v + 1 exists, belongs to this sequence and to this workgroup)
      const uint32_t next = slotcls[i + 1u];
      k[3] = next & 15u;
      k[4] = (next >> 4) & 15u;
    } else
    {
      if (3u * j + 3u < len)
      {
        k[3] = sf_classof(&t, chars, pos, len, 3u * j + 3u, &err);
      }
      if (3u * j + 4u < len)
      {
        k[4] = sf_classof(&t, chars, pos, len, 3u * j + 4u, &err);
      }
    }
    const uint64_t n0 = vsa_sf_framelength(len, 0),
                   n1 = vsa_sf_framelength(len, 1),
                   n2 = vsa_sf_framelength(len, 2);
    uint64_t fstart[VSA_SF_FRAMES], flen[3] = {n0, n1, n2};
    fstart[0] = pbase;
    fstart[1] = fstart[0] + n0 + 1u;
    fstart[2] = fstart[1] + n1 + 1u;
    fstart[3] = fstart[2] + n2 + 1u;
    fstart[4] = fstart[3] + n0 + 1u;
    fstart[5] = fstart[4] + n1 + 1u;
    // the five bases at two bits each, first base lowest (low) and first
    // base highest (high): six bits of either are the code of a codon of
    // plain bases read backward and forward; plain = one bit per plain base
    uint32_t low = 0, high = 0, plain = 0;
#pragma unroll
    for (uint32_t c = 0; c < 5u; c++)
    {
      const uint32_t base = (uint32_t) __builtin_ctz(k[c] | 16u) & 3u;
      low |= base << (2u * c);
      high |= base << (2u * (4u - c));
      plain |= (__builtin_popcount(k[c]) == 1 ? 1u : 0u) << c;
    }
#pragma unroll
    for (uint32_t g = 0; g < 3u; g++)
    {
      if (3u * j + g + 2u < len)
      {
        const uint32_t r = vsa_sf_reverseframe(len, g);
        uint8_t fwd, rev;
        if (((plain >> g) & 7u) == 7u)
        {
          fwd = t.mapped[(high >> (2u * (2u - g))) & 63u];
          rev = t.mapped[((low >> (2u * g)) & 63u) ^ VSA_SF_COMPLEMENT];
        } else
        {
          fwd = t.symbolmap[vsa_sf_codon(t.aminos, 1, k[g], k[g + 1],
                                         k[g + 2])];
          rev = t.symbolmap[vsa_sf_codon(t.aminos, 0, k[g + 2], k[g + 1],
                                         k[g])];
        }
        // (a code in [numofchars, 253]: no symbol of the index's alphabet)
        if (err == 0 && ((uint32_t) fwd - t.numofchars <=
                             VSA_UNDEFBWT - t.numofchars ||
                         (uint32_t) rev - t.numofchars <=
                             VSA_UNDEFBWT - t.numofchars))
        {
          err = SF_ERR_UNMAPPED;
        }
        protein[fstart[g] + j] = fwd;
        // (r as a switch: no indexing of the register arrays by a variable)
        const uint64_t rstart = r == 0 ? fstart[3]
                                : r == 1 ? fstart[4] : fstart[5],
                       rlen = r == 0 ? flen[0] : r == 1 ? flen[1] : flen[2];
        protein[rstart + (rlen - 1u - j)] = rev;
      }
    }
    if (UNIFORM)
    {
      // The separators, written where their neighbours are written: a pass
      // of its own leaves every line of the batch partly written twice.  The
      // first slot of a sequence closes its reverse frames (whose last
      // symbols it holds), the last slot its forward frames; an empty frame
      // is closed with them.  Not the one behind the last frame of all.
      if (j == 0)
      {
        protein[fstart[3] + n0] = (uint8_t) VSA_SEPARATOR;
        protein[fstart[4] + n1] = (uint8_t) VSA_SEPARATOR;
        if (fstart[5] + n2 < lay.nsymbols)
        {
          protein[fstart[5] + n2] = (uint8_t) VSA_SEPARATOR;
        }
      }
      if (j + 1u == nslots)
      {
        protein[fstart[0] + n0] = (uint8_t) VSA_SEPARATOR;
        protein[fstart[1] + n1] = (uint8_t) VSA_SEPARATOR;
        protein[fstart[2] + n2] = (uint8_t) VSA_SEPARATOR;
      }
    }
    if (err != 0)
    {
      atomicMax(errflag, err);
    }
  }
}

// pstart / plength / dnalength of a uniform batch, in closed form (the
// separators: k_sf_translate)
__global__ void __launch_bounds__(256)
k_sf_uniform_layout(uint64_t nq, uint64_t m, uint64_t span,
                    uint64_t *__restrict__ pstart,
                    uint64_t *__restrict__ plength,
                    uint64_t *__restrict__ dnalength)
{
  const uint64_t i = vsa_bid() * 256 + threadIdx.x;
  if (i < VSA_SF_FRAMES * nq)
  {
    const uint64_t s = i / VSA_SF_FRAMES;
    const uint32_t frame = (uint32_t) (i - s * VSA_SF_FRAMES);
    const uint64_t start = vsa_sf_framestart(s * span, m, frame),
                   flen = vsa_sf_framelength(m, frame);
    pstart[i] = start;
    plength[i] = flen;
    if (frame == 0)
    {
      dnalength[s] = m;
    }
  }
}

// the separator behind every frame but the last
__global__ void __launch_bounds__(256)
k_sf_separators(const uint64_t *__restrict__ pstart,
                const uint64_t *__restrict__ plength, uint64_t nframes,
                uint8_t *__restrict__ protein)
{
  const uint64_t i = vsa_bid() * 256 + threadIdx.x;
  if (i + 1u < nframes)
  {
    protein[pstart[i] + plength[i]] = (uint8_t) VSA_SEPARATOR;
  }
}

__global__ void __launch_bounds__(256)
k_sf_convert(const vsa_match *__restrict__ in, uint64_t n,
             const uint64_t *__restrict__ dnalength, uint64_t numofdna,
             uint64_t offset, vsa_match *__restrict__ out,
             uint8_t *__restrict__ reverse, uint32_t *__restrict__ bad)
{
  const uint64_t i = vsa_bid() * 256 + threadIdx.x;
  if (i < n)
  {
    const vsa_match m = in[i];
    const uint64_t q = m.queryseq - offset;
    vsa_match o = m;
    uint8_t rev = 0;
    if (m.queryseq < offset || q / VSA_SF_FRAMES >= numofdna ||
        vsa_sf_convert(&m, q, dnalength[q / VSA_SF_FRAMES],
                       offset / VSA_SF_FRAMES, &o, &rev) != 0)
    {
      atomicMax(bad, 1u);
    }
    out[i] = o;
    reverse[i] = rev;
  }
}

int maketables(uint32_t transnum, const uint8_t symbolmap[256], SfTables *t)
{
  vsa_sf_aminos(transnum, t->aminos);
  memcpy(t->symbolmap, symbolmap, 256);
  for (int c = 0; c < 256; c++)
  {
    t->cls[c] = (uint8_t) vsa_sf_class((uint8_t) c);
  }
  t->numofchars = 0;
  for (int c = 0; c < 256; c++)
  {
    if (symbolmap[c] < VSA_UNDEFBWT && symbolmap[c] + 1u > t->numofchars)
    {
      t->numofchars = symbolmap[c] + 1u;
    }
  }
  for (int c = 0; c < 64; c++)
  {
    t->mapped[c] = symbolmap[t->aminos[c]];
  }
  return 0;
}

// the reference's message for the first error of a batch: the host
// translation meets it first where the reference does
int hostmessage(uint32_t transnum, const uint8_t *chars, uint64_t nchars,
                const uint64_t *start, const uint64_t *length, uint64_t nq,
                const uint8_t symbolmap[256], uint64_t nsymbols)
{
  std::vector<uint8_t> protein(nsymbols + 1);
  std::vector<uint64_t> ps(VSA_SF_FRAMES * nq + 1), pl(VSA_SF_FRAMES * nq + 1);
  uint64_t got = 0;
  const int rc = vsa_translate_host(transnum, chars, nchars, start, length, nq,
                                    symbolmap, protein.data(), nsymbols,
                                    ps.data(), pl.data(), &got);
  if (rc == 0)
  {
    VSA_ERROR("the translation kernel reports an error the host translation "
              "does not find");
    return -100;
  }
  return rc;
}

// a batch of 6 nq sequences with room for its symbols, nothing laid out
int newbatch(uint64_t nq, uint64_t nsymbols, int device, vsa_queries **out)
{
  vsa_queries *q = new vsa_queries;
  q->device = device;
  q->nq = VSA_SF_FRAMES * nq;
  q->nsymbols = nsymbols;
  q->seqoffset = 0;
  q->symbols = nullptr;
  q->start = q->length = nullptr;
  q->minlength = q->maxlength = 0;
  q->uniform = q->dense = false; // ragged by construction: the byte paths
  *out = q;
  if (vsa_hip_malloc((void **) &q->symbols, nsymbols + VSA_QUERY_BACKPAD) !=
          hipSuccess ||
      vsa_hip_malloc((void **) &q->start, (q->nq + 1) * 8) != hipSuccess ||
      vsa_hip_malloc((void **) &q->length, (q->nq + 1) * 8) != hipSuccess ||
      vsa_hip_malloc((void **) &q->dnalength, (nq + 1) * 8) != hipSuccess ||
      hipMemset(q->symbols + nsymbols, 0xFF, VSA_QUERY_BACKPAD) != hipSuccess)
  {
    VSA_ERROR("vsa_queries_translate: no device memory for %lu symbols of "
              "%lu sequences", (unsigned long) nsymbols,
              (unsigned long) q->nq);
    vsa_queries_free(q);
    *out = nullptr;
    return -100;
  }
  return 0;
}

void summarise(vsa_queries *q)
{
  q->minlength = q->hlength.empty() ? 0 : ~0ull;
  q->maxlength = 0;
  for (uint64_t v : q->hlength)
  {
    q->minlength = std::min(q->minlength, v);
    q->maxlength = std::max(q->maxlength, v);
  }
}

// the kernels over a batch whose start / length / dnalength are in place
// (UNIFORM: are made here, on the device); *err = the error flag of the
// translation
template <bool UNIFORM>
int runkernels(vsa_queries *q, const uint8_t *d_chars, const SfLayout &lay,
               const SfTables &tables, uint32_t *err)
{
  DevBuf dtables, derr;
  Timer timer(nullptr);
  if (dtables.alloc(sizeof tables) != 0 || derr.alloc(4) != 0)
  {
    return -100;
  }
  VSA_HIP(hipMemcpyAsync(dtables.p, &tables, sizeof tables,
                         hipMemcpyHostToDevice, nullptr));
  VSA_HIP(hipMemsetAsync(derr.p, 0, 4, nullptr));
  timer.start();
  if (q->nq > 0 && UNIFORM)
  {
    k_sf_uniform_layout<<<vsa_grid((q->nq + 255) / 256), 256, 0, nullptr>>>(
        q->nq / VSA_SF_FRAMES, lay.m, lay.span, q->start, q->length,
        q->dnalength);
    if (lay.nslots == 0 && q->nsymbols > 0)
    {
      // reads without a codon: six empty frames each, separators only
      VSA_HIP(hipMemsetAsync(q->symbols, 0xFF, q->nsymbols, nullptr));
    }
  } else if (q->nq > 0)
  {
    k_sf_separators<<<vsa_grid((q->nq + 255) / 256), 256, 0, nullptr>>>(
        q->start, q->length, q->nq, q->symbols);
  }
  if (lay.nslots > 0)
  {
    const uint64_t blocks =
        (lay.nslots + VSA_TRANSLATE_TILE - 1) / VSA_TRANSLATE_TILE;
    k_sf_translate<UNIFORM>
        <<<vsa_grid(blocks), VSA_TRANSLATE_TILE, 0, nullptr>>>(
            d_chars, lay, dtables.as<SfTables>(), q->symbols,
            derr.as<uint32_t>());
  }
  timer.stop();
  VSA_HIP(hipGetLastError());
  VSA_HIP(hipMemcpy(err, derr.p, 4, hipMemcpyDeviceToHost));
  q->translate_ms = timer.ms();
  return 0;
}

} // namespace

extern "C" int vsa_queries_translate(uint32_t transnum,
                                     const uint8_t *dnachars, uint64_t nchars,
                                     const uint64_t *start,
                                     const uint64_t *length, uint64_t nq,
                                     const uint8_t symbolmap[256], int device,
                                     vsa_queries **protein)
{
  if (protein == nullptr || symbolmap == nullptr ||
      (nq > 0 && (start == nullptr || length == nullptr)) ||
      (nchars > 0 && dnachars == nullptr))
  {
    VSA_ERROR("vsa_queries_translate: NULL argument");
    return -1;
  }
  *protein = nullptr;
  if (vsa_transnum_check(transnum) != 0)
  {
    return -2;
  }
  // the layout: frames, compact sequences, the first sequence of every
  // workgroup
  std::vector<uint64_t> pstart(VSA_SF_FRAMES * nq), cstart, clen, cpbase,
      cslot;
  std::vector<uint32_t> blockfirst;
  uint64_t pos = 0, slots = 0;
  std::vector<uint64_t> plength(VSA_SF_FRAMES * nq);
  for (uint64_t s = 0; s < nq; s++)
  {
    if (start[s] > nchars || length[s] > nchars - start[s])
    {
      VSA_ERROR("sequence %lu [%lu, +%lu) lies outside the buffer of %lu "
                "characters", (unsigned long) s, (unsigned long) start[s],
                (unsigned long) length[s], (unsigned long) nchars);
      return -2;
    }
    const uint64_t len = length[s], nslots = len / 3u;
    if (nslots > 0)
    {
      if (cstart.size() >= 0xFFFFFFFFull)
      {
        VSA_ERROR("vsa_queries_translate: 2^32 sequences and more");
        return VSA_NOT_COVERED;
      }
      // the workgroups whose first slot lies in this sequence
      for (uint64_t b = (slots + VSA_TRANSLATE_TILE - 1) / VSA_TRANSLATE_TILE;
           b * VSA_TRANSLATE_TILE < slots + nslots; b++)
      {
        blockfirst.push_back((uint32_t) cstart.size());
      }
      cstart.push_back(start[s]);
      clen.push_back(len);
      cpbase.push_back(pos);
      cslot.push_back(slots);
      slots += nslots;
    }
    for (uint32_t f = 0; f < VSA_SF_FRAMES; f++)
    {
      pstart[VSA_SF_FRAMES * s + f] = pos;
      plength[VSA_SF_FRAMES * s + f] = vsa_sf_framelength(len, f);
      pos += vsa_sf_framelength(len, f) + 1u;
    }
  }
  const uint64_t nsymbols = nq > 0 ? pos - 1 : 0;
  cslot.push_back(slots);
  blockfirst.push_back(cstart.empty() ? 0 : (uint32_t) cstart.size() - 1);
  if (enter(device) != 0)
  {
    return -100;
  }
  vsa_queries *q = nullptr;
  if (newbatch(nq, nsymbols, device, &q) != 0)
  {
    return -100;
  }
  q->hlength.swap(plength);
  summarise(q);
  *protein = q;
  SfTables tables;
  maketables(transnum, symbolmap, &tables);
  const uint64_t nc = cstart.size();
  DevBuf dchars, dcstart, dclen, dcpbase, dcslot, dblockfirst;
  uint32_t err = 0;
  int rc = (dchars.alloc(nchars) || dcstart.alloc(nc * 8) ||
            dclen.alloc(nc * 8) || dcpbase.alloc(nc * 8) ||
            dcslot.alloc((nc + 1) * 8) ||
            dblockfirst.alloc(blockfirst.size() * 4))
               ? -100
               : 0;
  auto up = [&](void *dst, const void *src, size_t bytes) {
    if (rc == 0 && bytes > 0 &&
        hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess)
    {
      VSA_ERROR("vsa_queries_translate: upload failed");
      rc = -100;
    }
  };
  up(dchars.p, dnachars, nchars);
  up(dcstart.p, cstart.data(), nc * 8);
  up(dclen.p, clen.data(), nc * 8);
  up(dcpbase.p, cpbase.data(), nc * 8);
  up(dcslot.p, cslot.data(), (nc + 1) * 8);
  up(dblockfirst.p, blockfirst.data(), blockfirst.size() * 4);
  up(q->start, pstart.data(), q->nq * 8);
  up(q->length, q->hlength.data(), q->nq * 8);
  up(q->dnalength, length, nq * 8);
  if (rc == 0)
  {
    SfLayout lay;
    lay.cstart = dcstart.as<uint64_t>();
    lay.clen = dclen.as<uint64_t>();
    lay.cpbase = dcpbase.as<uint64_t>();
    lay.cslot = dcslot.as<uint64_t>();
    lay.blockfirst = dblockfirst.as<uint32_t>();
    lay.nslots = slots;
    lay.m = lay.span = lay.slotsper = lay.nsymbols = 0;
    rc = runkernels<false>(q, dchars.as<uint8_t>(), lay, tables, &err);
  }
  if (rc == 0 && err != 0)
  {
    rc = hostmessage(transnum, dnachars, nchars, start, length, nq, symbolmap,
                     nsymbols);
  }
  if (rc != 0)
  {
    vsa_queries_free(q);
    *protein = nullptr;
  }
  return rc;
}

extern "C" int vsa_queries_translate_device(uint32_t transnum,
                                            const void *device_chars,
                                            uint64_t nq, uint32_t m,
                                            const uint8_t symbolmap[256],
                                            int device, vsa_queries **protein)
{
  if (protein == nullptr || symbolmap == nullptr ||
      (nq > 0 && m > 0 && device_chars == nullptr))
  {
    VSA_ERROR("vsa_queries_translate_device: NULL argument");
    return -1;
  }
  *protein = nullptr;
  if (vsa_transnum_check(transnum) != 0)
  {
    return -2;
  }
  if (enter(device) != 0)
  {
    return -100;
  }
  const uint64_t span = vsa_sf_span(m), nsymbols = nq > 0 ? nq * span - 1 : 0;
  vsa_queries *q = nullptr;
  if (newbatch(nq, nsymbols, device, &q) != 0)
  {
    return -100;
  }
  q->hlength.resize(VSA_SF_FRAMES * nq);
  for (uint64_t i = 0; i < VSA_SF_FRAMES * nq; i++)
  {
    q->hlength[i] = vsa_sf_framelength(m, (uint32_t) (i % VSA_SF_FRAMES));
  }
  summarise(q);
  *protein = q;
  SfTables tables;
  maketables(transnum, symbolmap, &tables);
  SfLayout lay;
  lay.cstart = lay.clen = lay.cpbase = lay.cslot = nullptr;
  lay.blockfirst = nullptr;
  lay.m = m;
  lay.span = span;
  lay.nsymbols = nsymbols;
  lay.slotsper = m / 3u;
  lay.nslots = nq * lay.slotsper;
  uint32_t err = 0;
  int rc = runkernels<true>(q, (const uint8_t *) device_chars, lay, tables,
                            &err);
  if (rc == 0 && err != 0)
  {
    // the message: from the characters, on the host
    std::vector<uint8_t> chars(nq * (uint64_t) m);
    std::vector<uint64_t> start(nq), length(nq, (uint64_t) m);
    for (uint64_t s = 0; s < nq; s++)
    {
      start[s] = s * m;
    }
    if (hipMemcpy(chars.data(), device_chars, chars.size(),
                  hipMemcpyDeviceToHost) != hipSuccess)
    {
      VSA_ERROR("vsa_queries_translate_device: download failed");
      rc = -100;
    } else
    {
      rc = hostmessage(transnum, chars.data(), chars.size(), start.data(),
                       length.data(), nq, symbolmap, nsymbols);
    }
  }
  if (rc != 0)
  {
    vsa_queries_free(q);
    *protein = nullptr;
  }
  return rc;
}

extern "C" int vsa_queries_download(const vsa_queries *q, uint8_t *symbols,
                                    uint64_t *start, uint64_t *length)
{
  if (q == nullptr)
  {
    VSA_ERROR("vsa_queries_download: NULL argument");
    return -1;
  }
  if (q->rows != nullptr && !q->bytesvalid)
  {
    VSA_ERROR("vsa_queries_download: the bytes of this packed batch have not "
              "been made");
    return -2;
  }
  if (vsa_set_device(q->device) != 0)
  {
    return -100;
  }
  if (symbols != nullptr && q->nsymbols > 0)
  {
    VSA_HIP(hipMemcpy(symbols, q->symbols, q->nsymbols,
                      hipMemcpyDeviceToHost));
  }
  if (start != nullptr && q->nq > 0)
  {
    VSA_HIP(hipMemcpy(start, q->start, q->nq * 8, hipMemcpyDeviceToHost));
  }
  if (length != nullptr && q->nq > 0)
  {
    VSA_HIP(hipMemcpy(length, q->length, q->nq * 8, hipMemcpyDeviceToHost));
  }
  return 0;
}

extern "C" int vsa_translated_convert(const vsa_result *result,
                                      const vsa_queries *protein,
                                      vsa_result **queryview,
                                      uint8_t *reverse, uint64_t capacity)
{
  if (result == nullptr || protein == nullptr || queryview == nullptr)
  {
    VSA_ERROR("vsa_translated_convert: NULL argument");
    return -1;
  }
  *queryview = nullptr;
  if (result->packbits != 0)
  {
    VSA_ERROR("vsa_translated_convert: a packed candidate result has no "
              "records to convert");
    return VSA_NOT_COVERED;
  }
  if (result->extended)
  {
    VSA_ERROR("vsa_translated_convert: lists of extended seeds "
              "(VSA_SINK_QUERY_HAMMING, VSA_SINK_SELF_HAMMING, "
              "VSA_SINK_QUERY_EDIST, VSA_SINK_SELF_EDIST) are not covered");
    return VSA_NOT_COVERED;
  }
  if (protein->dnalength == nullptr)
  {
    VSA_ERROR("vsa_translated_convert: the batch is not a six-frame "
              "translation");
    return -2;
  }
  if (protein->seqoffset % VSA_SF_FRAMES != 0)
  {
    VSA_ERROR("the offset %lu of a six-frame batch is no multiple of 6",
              (unsigned long) protein->seqoffset);
    return -2;
  }
  if (result->device != protein->device)
  {
    VSA_ERROR("vsa_translated_convert: list on device %d, batch on device %d",
              result->device, protein->device);
    return -2;
  }
  if (enter(result->device) != 0)
  {
    return -100;
  }
  const uint64_t n = result->count;
  ResultGuard guard{newresult(result->device)};
  vsa_result *res = guard.r;
  DevBuf drev, dbad;
  Timer timer(nullptr);
  uint32_t bad = 0;
  res->count = res->stats.count = n;
  if (n > 0)
  {
    if (vsa_dev_alloc((void **) &res->matches, n * sizeof(vsa_match)) != 0 ||
        drev.alloc(n) != 0 || dbad.alloc(4) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemsetAsync(dbad.p, 0, 4, nullptr));
    timer.start();
    k_sf_convert<<<vsa_grid((n + 255) / 256), 256, 0, nullptr>>>(
        result->matches, n, protein->dnalength, protein->nq / VSA_SF_FRAMES,
        protein->seqoffset, res->matches, drev.as<uint8_t>(),
        dbad.as<uint32_t>());
    timer.stop();
    VSA_HIP(hipGetLastError());
    VSA_HIP(hipMemcpy(&bad, dbad.p, 4, hipMemcpyDeviceToHost));
    if (bad != 0)
    {
      VSA_ERROR("vsa_translated_convert: a record does not lie in a frame of "
                "the %lu DNA sequences",
                (unsigned long) (protein->nq / VSA_SF_FRAMES));
      return -2;
    }
    res->stats.total_device_ms = timer.ms();
    res->stats.sumlength = 3u * result->stats.sumlength;
    if (reverse != nullptr && capacity > 0)
    {
      VSA_HIP(hipMemcpy(reverse, drev.p, std::min(n, capacity),
                        hipMemcpyDeviceToHost));
    }
  }
  *queryview = res;
  guard.r = nullptr;
  return 0;
}
