// The driver of the extensions of exact seeds (extend.hip: -h K,
// extend_edist.hip: -e K, extend_xdrop.hip: -hxdrop X / -exdrop X), stated
// ONCE: what an entry refuses, the seed list
// it takes, the result it keeps, the E-value table on the device, the stable
// compaction of the kept records and the three forms of an entry -- a seed
// list, the seeds of a query batch, the seeds of the index against itself.
// Included inside the unnamed namespace of each unit, behind
// tile_compact.inc and the rules, so there is no object file and no symbol
// of its own.  A unit defines its kind, a struct with
//
//   cap                 the largest bound (distance, or X) of the device path
//   checkbound(who, b)  what the kind refuses of a bound b >= 1; a kind whose
//                       device path has a cap below what its host entry takes
//                       answers capbound<Kind>, which says so through
//   hosttakes(buf, n)   "vsa_..._host takes ..."
//   seedlength(L, b, S) the seed length rule of the kind
//   evalues             does the choice of the kind read the E-value table
//                       (is it made and uploaded)?
//   hequot              do the factors of the edit distances go up with it?
//   Stage               the scratch and the kernels between the seed list and
//                       the kept records, with
//     prepare(c, tall)            what comes before the buffers of the driver
//     run(c, recs, keep, counters, tall, tsearch)
//                                 ... and behind them: counters zeroed, the
//                                 kernels under tsearch; a record and a keep
//                                 flag per seed, the counters below
//     stats(st)                   the times of its own, the stream at rest
//                       The stage opens `tall` where its timed work begins;
//                       the driver closes it behind the compaction.
//
// and forwards its entries to extend_list, extend_queries and extend_self.

// words of the counters: what the stage counts for stats.searches, seeds
// that do not fit, sum of the lengths of the matches
#define EXT_NSTAGE 0
#define EXT_NMISFIT 1
#define EXT_SUMLENGTH 2
#define EXT_NCOUNTERS 3

// vsa_ext_word for `valid` >= 8 as one load
__device__ __forceinline__ uint64_t ext_word(const uint8_t *p, int left,
                                             uint64_t t0, uint64_t valid)
{
  if (valid < 8)
  {
    return vsa_ext_word(p, left, t0, valid);
  }
  return left ? __builtin_bswap64(vsa_load8(p - t0 - 7)) : vsa_load8(p + t0);
}

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

// a checked call, as a stage sees it
struct ExtCall
{
  const char *who;
  const vsa_index *index;
  const vsa_queries *queries; // the batch the seeds refer to, or -- self
  const vsa_result *seeds;    // count > 0
  int self;
  uint64_t leastlength, maxdist;
  uint64_t seedlength; // by the seed length rule of the kind
  vsa_selrules ev;     // the E-value table up to line maxdist, where the
                       // kind reads one
};

// a bound above the cap of the device path, where the host entry takes more
template <class Kind>
int capbound(const char *who, uint64_t maxdist)
{
  if (maxdist > Kind::cap)
  {
    char host[64];
    Kind::hosttakes(host, sizeof host);
    VSA_ERROR("%s: distance bound %lu: up to %u are covered on the device "
              "(%s)", who, (unsigned long) maxdist, Kind::cap, host);
    return VSA_NOT_COVERED;
  }
  return 0;
}

// what every entry refuses before anything is run or kept
template <class Kind>
int checkbounds(const char *who, const vsa_index *index,
                const vsa_queries *queries, uint64_t leastlength,
                uint64_t maxdist)
{
  if (leastlength == 0 || maxdist == 0)
  {
    VSA_ERROR("%s: a least length and a distance bound of at least 1", who);
    return -2;
  }
  const int rc = Kind::checkbound(who, maxdist);
  if (rc != 0)
  {
    return rc;
  }
  if (index->n >= 0xFFFFFFF0ull ||
      (queries != nullptr && queries->maxlength >= 0xFFFFFFF0ull))
  {
    VSA_ERROR("%s: texts and query sequences below 2^32 - 16 symbols are "
              "covered", who);
    return VSA_NOT_COVERED;
  }
  if (queries != nullptr && queries->device != index->device)
  {
    VSA_ERROR("%s: queries on device %d, index on device %d", who,
              queries->device, index->device);
    return -2;
  }
  return 0;
}

// the E-value table up to line K on the device, with the factors of the edit
// distances where the kind reads them (kurtz/evalues.c:315-420), as the sink
// and the selection make them
template <class Kind>
int evaluetable(const char *who, const vsa_index *index, uint64_t maxdist,
                DevBuf &dtable, DevBuf &dlines, DevBuf &dquot,
                vsa_selrules &ev)
{
  vsa_evalues hev;
  vsa_evalues_init(&hev, index->numofchars);
  if (vsa_evalues_extend(&hev, (int64_t) maxdist) != 0)
  {
    vsa_evalues_free(&hev);
    VSA_ERROR("out of memory");
    return -101;
  }
  double hequot[Kind::cap + 1];
  for (uint64_t d = 0; Kind::hequot && d <= maxdist; d++)
  {
    hequot[d] = vsa_evalues_hequot((int64_t) d);
  }
  const size_t tbytes = (size_t) hev.nexttab * 8,
               lbytes = (size_t) (maxdist + 2) * 8,
               qbytes = Kind::hequot ? (size_t) (maxdist + 1) * 8 : 0;
  int rc = (dtable.alloc(tbytes) != 0 || dlines.alloc(lbytes) != 0 ||
            (qbytes > 0 && dquot.alloc(qbytes) != 0))
               ? -100
               : 0;
  if (rc == 0 &&
      (hipMemcpy(dtable.p, hev.table, tbytes, hipMemcpyHostToDevice) !=
           hipSuccess ||
       hipMemcpy(dlines.p, hev.linestart, lbytes, hipMemcpyHostToDevice) !=
           hipSuccess ||
       (qbytes > 0 &&
        hipMemcpy(dquot.p, hequot, qbytes, hipMemcpyHostToDevice) !=
            hipSuccess)))
  {
    VSA_ERROR("%s: upload of the E-value table failed", who);
    rc = -100;
  }
  vsa_evalues_free(&hev);
  ev.table = dtable.as<double>();
  ev.linestart = dlines.as<int64_t>();
  ev.hequot = dquot.as<double>();
  ev.nlines = (int64_t) maxdist + 1;
  return rc;
}

// the seeds of `seeds` extended in the index and -- self == 0 -- in the batch
// they refer to; the arguments have been checked
template <class Kind>
int extend(const char *who, const vsa_index *index,
           const vsa_queries *queries, const vsa_result *seeds, int self,
           uint64_t leastlength, uint64_t maxdist, uint64_t seedlength,
           vsa_result **result)
{
  if (seeds->packbits != 0)
  {
    VSA_ERROR("%s: a packed candidate result has no records to extend", who);
    return VSA_NOT_COVERED;
  }
  if (seeds->extended)
  {
    VSA_ERROR("%s: the list holds extended seeds already", who);
    return VSA_NOT_COVERED;
  }
  if (seeds->count >= (1ull << 31))
  {
    VSA_ERROR("%s: %lu seeds: fewer than 2^31 are covered", who,
              (unsigned long) seeds->count);
    return VSA_NOT_COVERED;
  }
  if (seeds->device != index->device)
  {
    VSA_ERROR("%s: seeds on device %d, index on device %d", who,
              seeds->device, index->device);
    return -2;
  }
  if (enter(index->device) != 0)
  {
    return -100;
  }
  vsa_result *res = newresult(index->device);
  ResultGuard guard = {res};
  res->extended = true;
  res->stats.candidates = seeds->count;
  if (seeds->count == 0)
  {
    guard.r = nullptr;
    *result = res;
    return 0;
  }
  if (!self && vsa_queries_bytes(queries, nullptr) != 0)
  {
    return -100;
  }
  DevBuf dtable, dlines, dquot;
  ExtCall c;
  memset(&c, 0, sizeof c);
  if (Kind::evalues)
  {
    const int rc = evaluetable<Kind>(who, index, maxdist, dtable, dlines,
                                     dquot, c.ev);
    if (rc != 0)
    {
      return rc;
    }
  }
  int rc = 0;
  c.who = who;
  c.index = index;
  c.queries = queries;
  c.seeds = seeds;
  c.self = self;
  c.leastlength = leastlength;
  c.maxdist = maxdist;
  c.seedlength = Kind::seedlength(leastlength, maxdist, seedlength);

  const uint64_t nseeds = seeds->count;
  typename Kind::Stage stage;
  DevBuf counters, recs, keep, offsets, out;
  Timer tall(nullptr), tsearch(nullptr);
  if ((rc = stage.prepare(c, tall)) != 0)
  {
    return rc;
  }
  if (counters.alloc(EXT_NCOUNTERS * 8) != 0 ||
      recs.alloc(nseeds * sizeof(vsa_match)) != 0 || keep.alloc(nseeds) != 0)
  {
    return -100;
  }
  if ((rc = stage.run(c, recs.as<vsa_match>(), keep.as<uint8_t>(),
                      counters.as<unsigned long long>(), tall, tsearch)) != 0)
  {
    return rc;
  }
  KeptRecords f = {keep.as<uint8_t>(), recs.as<vsa_match>(), nullptr};
  uint64_t nout = 0;
  if (tc_count<1, 1>(f, nseeds, offsets, &nout) != 0)
  {
    return -100;
  }
  uint64_t words[EXT_NCOUNTERS];
  VSA_HIP(hipMemcpy(words, counters.p, sizeof words, hipMemcpyDeviceToHost));
  if (words[EXT_NMISFIT] != 0)
  {
    VSA_ERROR("%s: %lu seeds do not fit the index or their query sequence",
              who, (unsigned long) words[EXT_NMISFIT]);
    return -2;
  }
  if (nout > 0)
  {
    if (out.alloc(nout * sizeof(vsa_match)) != 0)
    {
      return -100;
    }
    f.out = out.as<vsa_match>();
    if (tc_emit<1>(f, nseeds, offsets) != 0)
    {
      return -100;
    }
  }
  tall.stop();
  VSA_HIP(hipStreamSynchronize(nullptr));
  res->count = nout;
  res->matches = nout > 0 ? (vsa_match *) out.release() : nullptr;
  res->stats.count = nout;
  res->stats.sumlength = words[EXT_SUMLENGTH];
  res->stats.searches = words[EXT_NSTAGE];
  res->stats.search_kernel_ms = tsearch.ms();
  res->stats.total_device_ms = tall.ms();
  stage.stats(res->stats);
  guard.r = nullptr;
  *result = res;
  return 0;
}

// ---- the three forms of an entry -------------------------------------------

// the bounds, then `run` on the batch (palindromic: on its reverse
// complement, which lives as long as the call)
template <class Kind, class Run>
int onbatch(const char *who, const vsa_index *index,
            const vsa_queries *queries, int palindromic, uint64_t leastlength,
            uint64_t maxdist, Run run)
{
  int rc = checkbounds<Kind>(who, index, queries, leastlength, maxdist);
  if (rc != 0)
  {
    return rc;
  }
  vsa_queries *rcq = nullptr;
  if (palindromic &&
      (rc = vsa_queries_reverse_complement(queries, &rcq)) != 0)
  {
    return rc;
  }
  rc = run(palindromic ? rcq : queries);
  vsa_queries_free(rcq);
  return rc;
}

// a seed list and the layout it was made under
template <class Kind>
int extend_list(const char *who, const vsa_index *index,
                const vsa_queries *queries, const vsa_result *seeds,
                const vsa_sinkparams *layout, int palindromic,
                uint64_t leastlength, uint64_t maxdist, uint64_t seedlength,
                vsa_result **result)
{
  if (index == nullptr || seeds == nullptr || layout == nullptr ||
      result == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  *result = nullptr;
  const bool self = layout->kind == VSA_SINK_SELF;
  if ((!self && layout->kind != VSA_SINK_QUERY) ||
      self != (queries == nullptr) || (self && palindromic))
  {
    VSA_ERROR("%s: the seeds of a query layout (VSA_SINK_QUERY, with their "
              "batch) or of a self layout (VSA_SINK_SELF, no batch, not "
              "palindromic) are extended", who);
    return -2;
  }
  return onbatch<Kind>(who, index, queries, palindromic, leastlength, maxdist,
                       [&](const vsa_queries *batch) {
                         return extend<Kind>(who, index, batch, seeds, self,
                                             leastlength, maxdist, seedlength,
                                             result);
                       });
}

// the exact matches of a batch of the seed length as seeds
template <class Kind>
int extend_queries(const char *who, const vsa_index *index,
                   const vsa_queries *queries, uint64_t leastlength,
                   uint64_t maxdist, uint64_t seedlength, int palindromic,
                   vsa_result **result)
{
  if (index == nullptr || queries == nullptr || result == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  *result = nullptr;
  return onbatch<Kind>(
      who, index, queries, palindromic, leastlength, maxdist,
      [&](const vsa_queries *batch) {
        vsa_result *seeds = nullptr;
        int rc = vsa_findquerymatches(
            index, batch, 0, 0,
            Kind::seedlength(leastlength, maxdist, seedlength), &seeds);
        if (rc == 0)
        {
          rc = extend<Kind>(who, index, batch, seeds, 0, leastlength, maxdist,
                            seedlength, result);
        }
        vsa_result_free(seeds);
        return rc;
      });
}

// the maximal repeats of the index of the seed length as seeds
template <class Kind>
int extend_self(const char *who, const vsa_index *index, uint64_t leastlength,
                uint64_t maxdist, uint64_t seedlength, vsa_result **result)
{
  if (index == nullptr || result == nullptr)
  {
    VSA_ERROR("%s: NULL argument", who);
    return -1;
  }
  *result = nullptr;
  int rc = checkbounds<Kind>(who, index, nullptr, leastlength, maxdist);
  if (rc != 0)
  {
    return rc;
  }
  vsa_result *seeds = nullptr;
  rc = vsa_findmaximalrepeats(
      index, Kind::seedlength(leastlength, maxdist, seedlength), &seeds);
  if (rc == 0)
  {
    rc = extend<Kind>(who, index, nullptr, seeds, 1, leastlength, maxdist,
                      seedlength, result);
  }
  vsa_result_free(seeds);
  return rc;
}
