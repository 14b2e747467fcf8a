// What does it cost on MI355X to throw the MUM candidates of the headline
// batch into buckets -- ONE store per candidate to an effectively random
// place of a staging area, with and without the returning atomicAdd on the
// bucket's counter that gives the place (candidate_sort.inc, k_cs_scatter)?
//
// n entries of 8 and of 16 bytes, bucket = hash of the entry's number, so
// neighbouring lanes never share a bucket (as reads in arrival order do not);
// without the atomic the place inside the bucket is a hash as well.  Read
// side: 12 bytes per entry, streamed (the first pass's arrays).
//
//   scatter_probe [entries [buckets [capacity]]]
//   hipcc --offload-arch=gfx950 -O3 -o _bin/scatter_probe scatter_probe.hip
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CK(x)                                                                 \
  do                                                                          \
  {                                                                           \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess)                                                     \
    {                                                                         \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

__device__ __forceinline__ uint64_t mix(uint64_t x)
{
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename ENTRY, bool ATOMIC>
__global__ void __launch_bounds__(256)
k_scatter(const uint32_t *__restrict__ len, const uint64_t *__restrict__ db,
          uint64_t n, uint32_t nbuckets, uint32_t cap,
          uint32_t *__restrict__ counts, ENTRY *__restrict__ staging)
{
  const uint64_t i = (uint64_t) blockIdx.x * 256 + threadIdx.x;
  if (i >= n)
  {
    return;
  }
  const uint64_t h = mix(i), key = (db[i] << 7) | len[i];
  const uint32_t b = (uint32_t) (h % nbuckets);
  uint32_t rank;
  if (ATOMIC)
  {
    rank = atomicAdd(&counts[b], 1u);
  } else
  {
    rank = (uint32_t) ((h >> 32) % cap);
  }
  if (rank < cap) // (never out of the staging area, whatever the hash does)
  {
    ENTRY e;
    if constexpr (sizeof(ENTRY) == 8)
    {
      e = key ^ h;
    } else
    {
      e = make_ulonglong2(key, h);
    }
    staging[(uint64_t) b * cap + rank] = e;
  }
}

template <typename ENTRY, bool ATOMIC>
static void row(const char *what, const uint32_t *len, const uint64_t *db,
                uint64_t n, uint32_t nbuckets, uint32_t cap, uint32_t *counts,
                void *staging)
{
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  const unsigned int grid = (unsigned int) ((n + 255) / 256);
  float best = 1e30f, sum = 0;
  const int reps = 6; // (the first one warms up and is not counted)
  for (int r = 0; r < reps; r++)
  {
    CK(hipMemsetAsync(counts, 0, (size_t) nbuckets * 4, 0));
    CK(hipEventRecord(a, 0));
    k_scatter<ENTRY, ATOMIC><<<grid, 256>>>(len, db, n, nbuckets, cap, counts,
                                            (ENTRY *) staging);
    CK(hipEventRecord(b, 0));
    CK(hipEventSynchronize(b));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, a, b));
    if (r > 0)
    {
      best = ms < best ? ms : best;
      sum += ms;
    }
  }
  const double mean = sum / (reps - 1);
  printf("%-44s %2zu-byte entries: best %7.1f us  mean %7.1f us  %6.1f G "
         "stores/s  (area %.0f MB)\n",
         what, sizeof(ENTRY), best * 1e3, mean * 1e3, n / (mean * 1e-3) / 1e9,
         (double) nbuckets * cap * sizeof(ENTRY) / 1e6);
  fflush(stdout);
  CK(hipEventDestroy(a));
  CK(hipEventDestroy(b));
}

int main(int argc, char **argv)
{
  const uint64_t n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 11600000ull;
  const uint32_t nbuckets = argc > 2 ? (uint32_t) atol(argv[2]) : 5722u;
  const uint32_t cap = argc > 3 ? (uint32_t) atol(argv[3]) : 4096u;
  uint32_t *len, *counts;
  uint64_t *db;
  void *staging;
  CK(hipMalloc((void **) &len, n * 4));
  CK(hipMalloc((void **) &db, n * 8));
  CK(hipMalloc((void **) &counts, (size_t) nbuckets * 4));
  CK(hipMalloc(&staging, (size_t) nbuckets * cap * 16));
  CK(hipMemset(len, 1, n * 4));
  CK(hipMemset(db, 1, n * 8));
  CK(hipMemset(staging, 0, (size_t) nbuckets * cap * 16));
  printf("%llu entries into %u buckets of capacity %u\n",
         (unsigned long long) n, nbuckets, cap);
  row<uint64_t, false>("one store, place from a hash", len, db, n, nbuckets,
                       cap, counts, staging);
  row<uint64_t, true>("one store, place from a returning atomicAdd", len, db,
                      n, nbuckets, cap, counts, staging);
  row<ulonglong2, false>("one store, place from a hash", len, db, n, nbuckets,
                         cap, counts, staging);
  row<ulonglong2, true>("one store, place from a returning atomicAdd", len,
                        db, n, nbuckets, cap, counts, staging);
  return 0;
}
