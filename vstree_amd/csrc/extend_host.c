/* Host side of the Hamming extension of exact seeds (include/vstree_amd.h,
   vsa_extend_hamming_host): hammingextend (kurtz/extendHD.c:166-374) for
   every seed of a list in host memory, by the rules of extend_rules.h, which
   the kernels of extend.hip read too.  No GPU involved; any distance bound;
   the seeds are dealt out to threads in pieces, the matches come out in the
   order of the seeds. */
#include <string.h>
#include "vstree_amd.h"
#include "extend_host_common.h"
#include "extend_rules.h"

#define WHO "vsa_extend_hamming_host"

typedef struct
{
  const vsa_sinkparams *layout;
  const uint8_t *text, *querysymbols;
  uint64_t leastlength, maxdist, seedlength;
  const vsa_selrules *ev;
} Job;

/* one side of seed: its look table, and the mismatches it offers */
static uint32_t scanside(const Job *j, int left, const vsa_ext_view *v1,
                         uint64_t pos1, const vsa_ext_view *v2, uint64_t pos2,
                         uint64_t length, uint64_t *look)
{
  vsa_ext_scan s;
  vsa_ext_plan plan;
  uint32_t h = 0;
  uint64_t t0;

  vsa_ext_begin(&s, look, 1, (uint32_t) j->maxdist, j->seedlength, left);
  if (vsa_ext_prepare(&s, v1, pos1, v2, pos2, length, &plan, &h) ==
      VSA_EXT_FIXED)
  {
    return h;
  }
  for (t0 = 0; t0 < plan.nsym; t0 += 8)
  {
    uint32_t sep;
    const uint64_t a = vsa_ext_word(plan.p1, left, t0, plan.nsym - t0),
                   b = vsa_ext_word(plan.p2, left, t0, plan.nsym - t0);
    const uint32_t marks = vsa_ext_marks8(a, b, &sep);

    if (vsa_ext_events(&s, &plan, t0, marks, sep))
    {
      return vsa_ext_end(&s);
    }
  }
  (void) vsa_ext_finish(&s, &plan);
  return vsa_ext_end(&s);
}

/* vsa_exthost_seed: scratch is the two look tables */
static int extendseed(const void *job, void *scratch, const vsa_match *m,
                      uint64_t where, vsa_match *o)
{
  const Job *j = (const Job *) job;
  const vsa_sinkparams *lay = j->layout;
  const int self = lay->kind == VSA_SINK_SELF;
  const vsa_ext_view text = {j->text, lay->totallength, 1, 1};
  uint64_t *look = (uint64_t *) scratch, *lookright = look + j->maxdist + 2;
  vsa_ext_view v2 = text;
  uint64_t pos2 = where, shift = 0, outlength = 0, dist = 0;
  uint32_t hleft, hright;

  if (!self)
  {
    v2.p = j->querysymbols + lay->querystart[where];
    v2.len = lay->querylength[where];
    v2.atstart = where == 0;
    v2.atend = where + 1 == lay->numofqueries;
    pos2 = m->querystart;
  }
  hleft = scanside(j, 1, &text, m->dbstart, &v2, pos2, m->length, look);
  hright = scanside(j, 0, &text, m->dbstart, &v2, pos2, m->length, lookright);
  if (!vsa_ext_choose(j->ev, m->length, j->leastlength, j->maxdist, look,
                      hleft, lookright, hright, 1, &shift, &outlength, &dist))
  {
    return 0;
  }
  o->length = VSA_HAMMING_PACK(outlength, dist);
  o->dbstart = m->dbstart - shift;
  o->queryseq = self ? m->queryseq - shift : m->queryseq;
  o->querystart = self ? 0 : m->querystart - shift;
  return 1;
}

static void *extendpiece(void *piece)
{
  return vsa_exthost_dopiece(piece, extendseed);
}

int vsa_extend_hamming_host(const vsa_sinkparams *layout, const uint8_t *text,
                            const uint8_t *querysymbols,
                            const vsa_match *seeds, uint64_t numofseeds,
                            uint64_t leastlength, uint64_t maxdist,
                            uint64_t seedlength, int threads,
                            vsa_match *matches, uint64_t capacity,
                            uint64_t *numofmatches)
{
  vsa_evalues ev;
  vsa_selrules evrules;
  Job job;
  int rc = vsa_exthost_check(WHO, layout, text, querysymbols, seeds,
                             numofseeds, leastlength, maxdist,
                             VSA_HAMMING_MAXDISTANCE, matches, capacity,
                             numofmatches);

  if (rc != 0 || numofseeds == 0)
  {
    return rc;
  }
  vsa_evalues_init(&ev, layout->numofchars);
  if (vsa_evalues_extend(&ev, (int64_t) maxdist) != 0)
  {
    vsa_evalues_free(&ev);
    return vsa_fail(-101, "out of memory");
  }
  memset(&evrules, 0, sizeof evrules);
  evrules.table = ev.table;
  evrules.linestart = ev.linestart;
  evrules.nlines = (int64_t) maxdist + 1;
  job.layout = layout;
  job.text = text;
  job.querysymbols = querysymbols;
  job.leastlength = leastlength;
  job.maxdist = maxdist;
  job.seedlength = vsa_ext_seedlength(leastlength, maxdist, seedlength);
  job.ev = &evrules;
  rc = vsa_exthost_extend(WHO, layout, seeds, numofseeds, threads, 1024,
                          extendpiece, &job,
                          2 * (maxdist + 2) * sizeof(uint64_t), matches,
                          capacity, numofmatches);
  vsa_evalues_free(&ev);
  return rc;
}
