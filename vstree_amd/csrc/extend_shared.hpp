// What the two extensions of exact seeds (extend.hip: -h K, extend_edist.hip:
// -e K) share on the host side of their translation units: the environment
// variable that forces one form of reading the symbols, and the compaction
// functor of the kept records.  Included inside the unnamed namespace of
// each unit, behind tile_compact.inc.

// VSA_EXTEND_STAGE: the symbols a lane looks at before it hands a side (a
// slide) over
uint32_t lanebudget()
{
  const char *e = getenv("VSA_EXTEND_STAGE");
  if (e != nullptr && strcmp(e, "lane") == 0)
  {
    return 0xFFFFFFFFu;
  }
  if (e != nullptr && strcmp(e, "long") == 0)
  {
    return 0;
  }
  return VSA_EXTEND_LANE_BUDGET;
}

// the kept records, in order
struct KeptRecords
{
  typedef NoPayload Payload;
  const uint8_t *keep;
  const vsa_match *in;
  vsa_match *out;

  __device__ int cls(uint64_t i, Payload &) const
  {
    return keep[i] != 0 ? 0 : -1;
  }
  __device__ void put(int, uint64_t rank, uint64_t i, const Payload &) const
  {
    out[rank] = in[i];
  }
};
