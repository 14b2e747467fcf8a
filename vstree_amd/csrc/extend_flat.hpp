// The query batch as the reference's Multiseq: one array with a separator
// between two sequences, wherever the sequences lie in the batch.  The
// extensions that step over the border of a sequence read it (extend_edist.hip:
// the fronts, extend_xdrop.hip: the generations and the trimming of
// xdropseedextend); extend_edist_rules.h says why views do not do.  Included
// inside the unnamed namespace of a unit behind extend_shared.hpp.  P is the
// unit's parameter struct, of which these members are read and written:
//   DevQueries q; const uint64_t *abs2; const uint8_t *s2; uint64_t n2;

template <class P>
__device__ __forceinline__ uint64_t flat_qlength(const P &p, uint64_t i)
{
  return p.q.uniformlen != 0 ? p.q.uniformlen : p.q.length[i];
}

// where sequence i of the batch begins in the query Multiseq
template <class P>
__device__ __forceinline__ uint64_t flat_qabs(const P &p, uint64_t i)
{
  return p.q.uniformlen != 0 ? i * ((uint64_t) p.q.uniformlen + 1)
                             : p.abs2[i];
}

#define FLAT_BLOCK 256

// one wavefront per sequence
template <class P>
__global__ void __launch_bounds__(FLAT_BLOCK)
k_flatten(P p, uint8_t *__restrict__ out)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwaves = vsa_nblocks() * (FLAT_BLOCK / 64);

  for (uint64_t i = vsa_bid() * (FLAT_BLOCK / 64) + (threadIdx.x >> 6);
       i < p.q.nq; i += nwaves)
  {
    const uint64_t len = flat_qlength(p, i);
    const uint8_t *src =
        p.q.symbols + (p.q.dense ? i * p.q.uniformlen : p.q.start[i]);
    uint8_t *dst = out + flat_qabs(p, i);
    for (uint64_t x = lane; x < len; x += 64)
    {
      dst[x] = src[x];
    }
    if (lane == 0 && i + 1 < p.q.nq)
    {
      dst[len] = (uint8_t) VSA_SEPARATOR;
    }
  }
}

// the Multiseq of `queries` into flat (16 bytes of slack behind it), the
// starts of a ragged batch into abs2; p.q, p.abs2, p.s2, p.n2 are set
template <class P>
int flatten_batch(const char *who, const vsa_queries *queries, P &p,
                  DevBuf &flat, DevBuf &abs2)
{
  p.q = devqueries(queries);
  const uint64_t nq = queries->nq;
  uint64_t total = 0;
  if (p.q.uniformlen != 0)
  {
    total = nq * ((uint64_t) p.q.uniformlen + 1) - (nq > 0 ? 1 : 0);
  } else
  {
    if (queries->hlength.size() != nq)
    {
      VSA_ERROR("%s: the batch has no host copy of its lengths", who);
      return -2;
    }
    std::vector<uint64_t> starts(nq);
    for (uint64_t i = 0; i < nq; i++)
    {
      starts[i] = total + (i > 0 ? 1 : 0);
      total = starts[i] + queries->hlength[i];
    }
    if (abs2.alloc(nq * 8) != 0)
    {
      return -100;
    }
    VSA_HIP(hipMemcpy(abs2.p, starts.data(), nq * 8, hipMemcpyHostToDevice));
    p.abs2 = abs2.as<uint64_t>();
  }
  if (flat.alloc(total + 16) != 0)
  {
    return -100;
  }
  const uint64_t blocks = std::min<uint64_t>(
      (nq + FLAT_BLOCK / 64 - 1) / (FLAT_BLOCK / 64), 65536);
  k_flatten<P><<<vsa_grid(blocks), FLAT_BLOCK, 0, nullptr>>>(
      p, flat.as<uint8_t>());
  VSA_HIP(hipGetLastError());
  p.s2 = flat.as<uint8_t>();
  p.n2 = total;
  return 0;
}
