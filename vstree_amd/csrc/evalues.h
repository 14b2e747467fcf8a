/*
  The E-value table of the host match sink (match_sink.c), for the other
  translation unit that needs the very same numbers: the match selection
  (select_host.c builds the tables its kernels read from it).
    inithammingEvalues, incprecomputehammingEvalues and the factors of
    incgetEvalue, kurtz/evalues.c:59-83,307-368,402-414
*/
#ifndef VSA_EVALUES_H
#define VSA_EVALUES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
  double probmatch, first;
  int64_t *linestart; /* nextline + 1 entries are valid */
  uint64_t nextline, alloclines;
  double *table;
  uint64_t nexttab, alloctab;
} vsa_evalues;

/* inithammingEvalues(&evalues, 1.0 / (mapsize - 1)), kurtz/evalues.c:307-314 */
void vsa_evalues_init(vsa_evalues *h, uint32_t numofchars);
void vsa_evalues_free(vsa_evalues *h);
/* lines 0 .. kmax of the table */
int vsa_evalues_extend(vsa_evalues *h, int64_t kmax);
/* the factor of incgetEvalue for an edit distance: averagequot[distance] up
   to 20, 1.31e7 * 2^(distance - 20) up to 120 (kurtz/evalues.c:59-83,
   402-414); the caller answers 0.0 beyond */
#define VSA_EVALUES_MAXEDIST 120
double vsa_evalues_hequot(int64_t distance);

#ifdef __cplusplus
}
#endif
#endif
