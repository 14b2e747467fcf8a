/*
  What the host files of the library share, stated ONCE: the message buffer
  with its size, a bounded text buffer, the checks of a layout with the view
  of a match they lead to (select_rules.h), and the checks of a list in host
  memory.  Plain C that the C++ units read too; static inline functions only,
  so there is no object file and no symbol of its own.
*/
#ifndef VSA_HOST_COMMON_H
#define VSA_HOST_COMMON_H
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "vstree_amd.h"
#include "select_rules.h"

/* ---- the message buffer (g_errbuf of api.hip, one per thread) ------------- */

#ifdef __cplusplus
extern "C" {
#endif
char *vsa_errbuf(void);
#ifdef __cplusplus
}
#endif
#define VSA_ERRBUF_SIZE 1024

/* the message, cut at the size of the buffer -> rc */
#ifdef __GNUC__
__attribute__((format(printf, 2, 3)))
#endif
static inline int vsa_fail(int rc, const char *fmt, ...)
{
  va_list ap;

  va_start(ap, fmt);
  vsnprintf(vsa_errbuf(), VSA_ERRBUF_SIZE, fmt, ap);
  va_end(ap);
  return rc;
}

/* ---- bounded text: the bytes that did not fit are counted, not written ---- */

typedef struct
{
  char *p;
  uint64_t cap, len;
} vsa_textbuf;

static inline void vsa_put(vsa_textbuf *t, const char *s, size_t n)
{
  if (t->len + n < t->cap)
  {
    memcpy(t->p + t->len, s, n);
  }
  t->len += n;
}

/* one formatted line of fewer than 512 bytes */
#ifdef __GNUC__
__attribute__((format(printf, 2, 3)))
#endif
static inline void vsa_putf(vsa_textbuf *t, const char *fmt, ...)
{
  char line[512];
  va_list ap;
  int n;

  va_start(ap, fmt);
  n = vsnprintf(line, sizeof line, fmt, ap);
  va_end(ap);
  if (n > 0)
  {
    vsa_put(t, line, n < (int) sizeof line ? (size_t) n : sizeof line - 1);
  }
}

/* the length of the text with its final 0 in place, or the message and -3 */
static inline int64_t vsa_endtext(vsa_textbuf *t, const char *who)
{
  if (t->len >= t->cap)
  {
    return vsa_fail(-3, "%s: %lu bytes do not fit a buffer of %lu", who,
                    (unsigned long) t->len + 1, (unsigned long) t->cap);
  }
  t->p[t->len] = '\0';
  return (int64_t) t->len;
}

/* ---- a layout and the view of a match under it ---------------------------- */

#define VSA_NEEDS_NOSELFPAL 1 /* lists of vmatch -p IDX are refused         */
#define VSA_NEEDS_SEQUENCES 2 /* numofsequences and, beyond one, markpos    */
#define VSA_NEEDS_QUERIES 4   /* querystart / querylength of a query layout */
#define VSA_NEEDS_CHARS 8     /* numofchars >= 2                            */

static inline int vsa_layout_selfpalindromic(const vsa_sinkparams *layout,
                                             const char *who)
{
  return layout->selfpalindromic
             ? vsa_fail(VSA_NOT_COVERED, "%s: lists of vmatch -p IDX "
                        "(selfpalindromic) are not covered", who)
             : 0;
}

/* The refusals every post-processing feature makes of a layout, in this
   order: selfpalindromic (where asked for), a six-frame translated batch, an
   incomplete layout.  0 and the base of the view of a match: no E-value is
   looked at, and the query Multiseq is the layout's own. */
static inline int vsa_layout_view(const vsa_sinkparams *layout,
                                  const char *who, int needs,
                                  vsa_selrules *view)
{
  if ((needs & VSA_NEEDS_NOSELFPAL) &&
      vsa_layout_selfpalindromic(layout, who) != 0)
  {
    return VSA_NOT_COVERED;
  }
  if (layout->kind == VSA_SINK_TRANSLATED ||
      layout->kind == VSA_SINK_TRANSLATED_COMPLETE)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: lists of a six-frame translated "
                    "batch (VSA_SINK_TRANSLATED) are not covered", who);
  }
  if (layout->kind == VSA_SINK_QUERY_HAMMING ||
      layout->kind == VSA_SINK_SELF_HAMMING ||
      layout->kind == VSA_SINK_QUERY_EDIST ||
      layout->kind == VSA_SINK_SELF_EDIST)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: lists of extended seeds "
                    "(VSA_SINK_QUERY_HAMMING, VSA_SINK_SELF_HAMMING, "
                    "VSA_SINK_QUERY_EDIST, VSA_SINK_SELF_EDIST) are not "
                    "covered", who);
  }
  if (layout->kind >= VSA_SINK_QUERY_HXDROP &&
      layout->kind <= VSA_SINK_SELF_EXDROP)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: lists of extended seeds "
                    "(VSA_SINK_QUERY_HXDROP, VSA_SINK_SELF_HXDROP, "
                    "VSA_SINK_QUERY_EXDROP, VSA_SINK_SELF_EXDROP) are not "
                    "covered", who);
  }
  if (layout->kind < VSA_SINK_COMPLETE ||
      layout->kind > VSA_SINK_APPROX_HAMMING || layout->totallength == 0 ||
      layout->totalquerylength + 1 > layout->totallength ||
      ((needs & VSA_NEEDS_CHARS) && layout->numofchars < 2) ||
      ((needs & VSA_NEEDS_SEQUENCES) &&
       (layout->numofsequences == 0 ||
        (layout->numofsequences > 1 && layout->markpos == NULL))) ||
      ((needs & VSA_NEEDS_QUERIES) && layout->kind != VSA_SINK_SELF &&
       layout->numofqueries > 0 &&
       (layout->querystart == NULL || layout->querylength == NULL)))
  {
    return vsa_fail(-2, "%s: incomplete layout", who);
  }
  memset(view, 0, sizeof *view);
  view->kind = layout->kind;
  view->noevalue = 1;
  view->totallength = (double) layout->totallength;
  if (layout->kind == VSA_SINK_SELF)
  {
    view->hasindexedqueries = layout->totalquerylength > 0;
    view->dblenplus1 = layout->totallength - layout->totalquerylength;
  } else
  {
    view->nq = layout->numofqueries;
    view->qstart = layout->querystart;
    view->qlen = layout->querylength;
  }
  return 0;
}

/* ---- a list in host memory ------------------------------------------------ */

/* n records at matches; noun ("records", "matches") != NULL: fewer than
   2^32 - 1 of them */
static inline int vsa_list_check(const char *who, const char *noun,
                                 const vsa_match *matches, uint64_t n)
{
  if (matches == NULL && n > 0)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (noun != NULL && n >= 0xFFFFFFFFull)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: %lu %s: only fewer than 2^32 - 1 "
                    "are covered", who, (unsigned long) n, noun);
  }
  return 0;
}

/* the D / P flag of record i -> *pal; a P record of a self list is refused */
static inline int vsa_list_flag(const char *who, int kind,
                                const uint8_t *palindromic, uint64_t i,
                                int *pal)
{
  *pal = palindromic != NULL && palindromic[i] != 0;
  return *pal && kind == VSA_SINK_SELF
             ? vsa_fail(VSA_NOT_COVERED, "%s: palindromic self matches are "
                        "the selfpalindromic form", who)
             : 0;
}

static inline int vsa_list_misfit(const char *who, uint64_t i)
{
  return vsa_fail(-2, "%s: record %lu does not fit the layout", who,
                  (unsigned long) i);
}

#endif
