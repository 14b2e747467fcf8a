/*
  What align_host.c needs of the sink (match_sink.c) to print the match line
  in front of an alignment: the parameters the sink was opened with, the
  E-value table brought up to a batch, a formatting cache per thread, one
  line, and the position of a text position in its sequence.  Not part of
  the public interface.
*/
#ifndef VSA_SINK_INTERNAL_H
#define VSA_SINK_INTERNAL_H
#include "vstree_amd.h"

#define VSA_SINK_LINEMAX 192 /* upper bound of one match line */

const vsa_sinkparams *vsa_sink_params_(const vsa_sink *s);
/* before the first vsa_sink_line_ of a batch, from one thread */
int vsa_sink_prepare_(vsa_sink *s, const vsa_match *matches, uint64_t n);
void *vsa_sink_cache_new_(void);
void vsa_sink_cache_free_(void *cache);
/* the line of m with its newline at o -> its end; o itself if the sink
   drops the match; NULL for a record outside the layout */
char *vsa_sink_line_(const vsa_sink *s, void *cache, const vsa_match *m,
                     char *o);
uint64_t vsa_sink_relpos_(const vsa_sink *s, uint64_t pos);

#endif
