/* What select.hip needs of select_host.c: the validated description of a
   selection with the tables its kernels read, and the -sort tail. */
#ifndef VSA_SELECT_INTERNAL_H
#define VSA_SELECT_INTERNAL_H
#include "select_rules.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
  vsa_selrules rules; /* host view: the pointers are host memory          */
  vsa_selectparams params;
  vsa_evalues ev;
  double *hequot;     /* rules.nlines entries                             */
  uint64_t *qstart, *qlen; /* owned copies (NULL for uniform batches)     */
} vsa_selctx;

/* checks layout and params (message and -2 / VSA_NOT_COVERED), copies the
   query Multiseq (qstart / qlen of nq sequences, or uniformlen != 0) and
   builds the first lines of the table */
int vsa_selctx_init(vsa_selctx *ctx, const vsa_sinkparams *layout,
                    const vsa_selectparams *params, uint64_t nq,
                    const uint64_t *qstart, const uint64_t *qlen,
                    uint32_t uniformlen, uint64_t seqoffset);
void vsa_selctx_free(vsa_selctx *ctx);
/* the table reaches the largest distance of a list (the querystart field of
   approximate layouts); 1 if it grew, 0 if not, < 0 on error */
int vsa_selctx_ensure(vsa_selctx *ctx, uint64_t maxdistance);

/* showbestmatchlist with a sort mode (Vmatch/procfinal.c:720-743): n records
   in best-first order with their flags and E-values are rearranged in place;
   returns the number that stay, *contained = the number removecontained
   dropped; < 0 on error */
int64_t vsa_select_sorttail(const vsa_selctx *ctx, vsa_match *matches,
                            uint8_t *flags, double *evalues, uint64_t n,
                            uint64_t *contained);

#ifdef __cplusplus
}
#endif
#endif
