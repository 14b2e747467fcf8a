/*
  Match clustering, host side: a fresh restatement of mirrorandsortmatches,
  gapclustermatches and overlapclustermatches (Vmatch/clpos.c:34-201) as the
  reference writes them -- two nested loops over the sorted references, the
  inner one left at the first successor out of reach -- and of the lines of
  domatchclustering (Vmatch/matchclust.c:10-128).  linkcluster, the numbering
  of showClusterSet and the order of addClusterEdge are those of
  cluster_host.c (vsa_cl_replay), over the matches as elements.
  vsa_matchcluster_host sends every edge through linkcluster;
  matchcluster.hip sends only the edges of the spanning forest it found
  through the same code.  No GPU involved.
*/
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "matchcluster_rules.h"
#include "erate_rules.h"
#include "host_common.h"

int vsa_mc_checklayout(const vsa_sinkparams *layout,
                       const vsa_matchclusterparams *params, const char *who,
                       vsa_selrules *rules, vsa_mcrules *mcrules)
{
  int rc;

  if (layout == NULL || params == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (params->mode == VSA_MATCHCLUSTER_ERATE)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: matchcluster erate (the edit "
                    "distance between the match substrings) is not covered "
                    "here: it needs the text (vsa_eratecluster_open, "
                    "vsa_eratecluster_host)", who);
  }
  if (params->mode != VSA_MATCHCLUSTER_GAP &&
      params->mode != VSA_MATCHCLUSTER_OVERLAP)
  {
    return vsa_fail(-2, "%s: illegal mode %d", who, params->mode);
  }
  if (params->mode == VSA_MATCHCLUSTER_GAP &&
      params->maxgapsize >= VSA_MC_MAXGAP)
  {
    return vsa_fail(-2, "%s: a gap size of %lu is beyond 2^62", who,
                    (unsigned long) params->maxgapsize);
  }
  if ((rc = vsa_layout_view(layout, who, VSA_NEEDS_NOSELFPAL |
                            VSA_NEEDS_QUERIES, rules)) != 0)
  {
    return rc;
  }
  mcrules->mode = params->mode;
  mcrules->maxgapsize = params->maxgapsize;
  mcrules->minpercentoverlap = params->minpercentoverlap;
  return 0;
}

/* domatchclustering and showclnum, matchclust.c:10-16,94 */
int64_t vsa_mc_format(uint64_t matches, const vsa_clresult *r, char *buffer,
                      uint64_t capacity)
{
  vsa_textbuf t = {buffer, capacity, 0};
  uint64_t c;

  vsa_putf(&t, "# cluster %lu matches\n", (unsigned long) matches);
  for (c = 0; c < r->clusters; c++)
  {
    vsa_putf(&t, "# create cluster %lu of size %lu\n", (unsigned long) c,
             (unsigned long) (r->clusterstart[c + 1] - r->clusterstart[c]));
  }
  return vsa_endtext(&t, "vsa_matchcluster_format");
}

/* showclelem and showedge with the two mcllinkinfo functions,
   matchclust.c:31-85, clpos.c:53-70 */
int64_t vsa_matchcluster_format_host(vsa_sink *sink, int mode,
                                     const uint64_t *member,
                                     const vsa_match *records, uint64_t size,
                                     const uint32_t *m0, const uint32_t *m1,
                                     const uint64_t *value, uint64_t nedges,
                                     char *buffer, uint64_t capacity)
{
  vsa_textbuf t = {buffer, capacity, 0};
  char line[512];
  uint64_t i;

  if (sink == NULL || buffer == NULL || (size > 0 && (member == NULL ||
      records == NULL)) || (nedges > 0 && (m0 == NULL || m1 == NULL ||
      value == NULL)))
  {
    return vsa_fail(-1, "vsa_matchcluster_format_host: NULL argument");
  }
  for (i = 0; i < size; i++)
  {
    int64_t w;
    vsa_putf(&t, "# id %lu\n", (unsigned long) member[i]);
    w = vsa_sink_format(sink, records + i, 1, line, sizeof line);
    if (w < 0)
    {
      return w;
    }
    vsa_put(&t, line, (size_t) w);
  }
  for (i = 0; i < nedges; i++)
  {
    if (mode == VSA_MATCHCLUSTER_GAP)
    {
      vsa_putf(&t, "# linked %lu and %lu with gapsize %lu\n",
               (unsigned long) m0[i], (unsigned long) m1[i],
               (unsigned long) value[i]);
    } else if (mode == VSA_MATCHCLUSTER_ERATE)
    {
      /* cluedistmlclinkinfo, cluedist.c:108-118 */
      const uint64_t edist = value[i] & 0xFFFFFFFFull,
                     minlen = value[i] >> 32;
      vsa_putf(&t, "# linked %lu and %lu with edit distance %lu (error rate "
               "%.2f%%)\n", (unsigned long) m0[i], (unsigned long) m1[i],
               (unsigned long) edist,
               100.00 * (double) edist / (double) minlen);
    } else
    {
      double overlap;
      memcpy(&overlap, value + i, 8);
      vsa_putf(&t, "# linked %lu and %lu with overlap percentage %.2f\n",
               (unsigned long) m0[i], (unsigned long) m1[i], overlap);
    }
  }
  return vsa_endtext(&t, "vsa_matchcluster_format_cluster");
}

/* ---- the references, sorted like glibc's qsort sorts them ---------------- */

typedef struct
{
  uint64_t start;
  uint32_t matchnum;
} Mref;

/* a merge sort that takes the left run on ties: equal starts keep the order
   of their index */
static void sortrefs(Mref *a, Mref *tmp, uint64_t n)
{
  uint64_t width, lo;

  for (width = 1; width < n; width *= 2)
  {
    for (lo = 0; lo < n; lo += 2 * width)
    {
      const uint64_t mid = lo + width < n ? lo + width : n,
                     hi = lo + 2 * width < n ? lo + 2 * width : n;
      uint64_t i = lo, j = mid, k = lo;
      while (i < mid && j < hi)
      {
        tmp[k++] = a[j].start < a[i].start ? a[j++] : a[i++];
      }
      while (i < mid)
      {
        tmp[k++] = a[i++];
      }
      while (j < hi)
      {
        tmp[k++] = a[j++];
      }
    }
    memcpy(a, tmp, (size_t) n * sizeof *a);
  }
}

typedef struct
{
  uint32_t *m0, *m1;
  uint64_t *value;
  uint64_t n, cap;
} Edges;

static int addedge(Edges *e, uint32_t a, uint32_t b, uint64_t value)
{
  if (e->n == e->cap)
  {
    const uint64_t cap = e->cap ? 2 * e->cap : 1024;
    uint32_t *m0 = realloc(e->m0, (size_t) cap * sizeof *m0);
    uint32_t *m1 = m0 ? realloc(e->m1, (size_t) cap * sizeof *m1) : NULL;
    uint64_t *v = m1 ? realloc(e->value, (size_t) cap * sizeof *v) : NULL;
    if (m0 != NULL)
    {
      e->m0 = m0;
    }
    if (m1 != NULL)
    {
      e->m1 = m1;
    }
    if (v == NULL)
    {
      return vsa_fail(-1, "out of memory");
    }
    e->value = v;
    e->cap = cap;
  }
  e->m0[e->n] = a;
  e->m1[e->n] = b;
  e->value[e->n++] = value;
  return 0;
}

/* the end of both host entries: the edges through linkcluster, and what the
   caller asked for of the result */
static int deliver(const char *who, uint64_t n, const Edges *edges,
                   vsa_matchclusterstats *st, vsa_matchclusterstats *stats,
                   uint64_t *clusterstart, uint64_t *members, uint64_t *label,
                   uint64_t *edgestart, uint32_t *m0, uint32_t *m1,
                   uint64_t *value, uint64_t edgecapacity, char *buffer,
                   uint64_t capacity, int64_t *written)
{
  const Edges e = *edges;
  vsa_clresult res;
  uint64_t *fill = NULL;
  uint64_t i;
  int64_t bytes = 0;
  int rc;

  memset(&res, 0, sizeof res);
  st->edges = e.n;
  if ((rc = vsa_cl_replay(n, e.m0, e.m1, e.n, &st->forestedges, &res)) != 0)
  {
    goto done;
  }
  st->clusters = res.clusters;
  st->inclusters = res.inclusters;
  if (stats != NULL)
  {
    *stats = *st;
  }
  if ((m0 != NULL || m1 != NULL || value != NULL) && e.n > edgecapacity)
  {
    rc = vsa_fail(-3, "%s: %lu edges, room for %lu", who,
                  (unsigned long) e.n, (unsigned long) edgecapacity);
    goto done;
  }
  if (buffer != NULL &&
      (bytes = vsa_mc_format(n, &res, buffer, capacity)) < 0)
  {
    rc = (int) bytes;
    goto done;
  }
  if (edgestart != NULL || m0 != NULL || m1 != NULL || value != NULL)
  {
    /* addClusterEdge (cluster.c:586-614): each cluster's part is filled
       from the back in the order of the edges */
    fill = calloc((size_t) res.clusters + 2, sizeof *fill);
    if (fill == NULL)
    {
      rc = vsa_fail(-1, "out of memory");
      goto done;
    }
    for (i = 0; i < e.n; i++)
    {
      fill[res.label[e.m0[i]] + 1]++;
    }
    for (i = 0; i < res.clusters; i++)
    {
      fill[i + 1] += fill[i];
    }
    if (edgestart != NULL)
    {
      memcpy(edgestart, fill, (size_t) (res.clusters + 1) * sizeof *fill);
    }
    for (i = 0; i < e.n; i++)
    {
      const uint64_t at = --fill[res.label[e.m0[i]] + 1];
      if (m0 != NULL)
      {
        m0[at] = e.m0[i];
      }
      if (m1 != NULL)
      {
        m1[at] = e.m1[i];
      }
      if (value != NULL)
      {
        value[at] = e.value[i];
      }
    }
  }
  if (clusterstart != NULL)
  {
    memcpy(clusterstart, res.clusterstart,
           (size_t) (res.clusters + 1) * sizeof *clusterstart);
  }
  if (members != NULL && res.inclusters > 0)
  {
    memcpy(members, res.members, (size_t) res.inclusters * sizeof *members);
  }
  if (label != NULL && n > 0)
  {
    memcpy(label, res.label, (size_t) n * sizeof *label);
  }
  if (written != NULL)
  {
    *written = bytes;
  }
done:
  vsa_cl_freeresult(&res);
  free(fill);
  return rc;
}

int vsa_matchcluster_host(const vsa_sinkparams *layout,
                          const vsa_matchclusterparams *params,
                          const vsa_match *matches, const uint8_t *palindromic,
                          uint64_t n, vsa_matchclusterstats *stats,
                          uint64_t *clusterstart, uint64_t *members,
                          uint64_t *label, uint64_t *edgestart, uint32_t *m0,
                          uint32_t *m1, uint64_t *value,
                          uint64_t edgecapacity, char *buffer,
                          uint64_t capacity, int64_t *written)
{
  static const char who[] = "vsa_matchcluster_host";
  vsa_selrules rules;
  vsa_mcrules mc;
  vsa_matchclusterstats st;
  Edges e = {NULL, NULL, NULL, 0, 0};
  Mref *ref = NULL, *tmp = NULL;
  uint64_t *length = NULL;
  uint64_t i, j;
  int rc = vsa_mc_checklayout(layout, params, who, &rules, &mc);

  if (rc != 0 || (rc = vsa_list_check(who, "matches", matches, n)) != 0)
  {
    return rc;
  }
  memset(&st, 0, sizeof st);
  st.matches = n;
  ref = malloc((size_t) (2 * n + 1) * sizeof *ref);
  tmp = malloc((size_t) (2 * n + 1) * sizeof *tmp);
  length = malloc((size_t) (n + 1) * sizeof *length);
  if (ref == NULL || tmp == NULL || length == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  for (i = 0; i < n; i++)
  {
    vsa_selvalues v;
    int pal;
    if ((rc = vsa_list_flag(who, layout->kind, palindromic, i, &pal)) != 0)
    {
      goto done;
    }
    if (vsa_sel_values(&rules, matches + i, pal, &v) != 0)
    {
      rc = vsa_list_misfit(who, i);
      goto done;
    }
    length[i] = v.length1;
    ref[2 * i].start = v.position1;
    ref[2 * i].matchnum = (uint32_t) i;
    ref[2 * i + 1].start = v.position2;
    ref[2 * i + 1].matchnum = (uint32_t) i;
  }
  sortrefs(ref, tmp, 2 * n);
  for (i = 0; i + 1 < 2 * n; i++)
  {
    const uint64_t len_i = length[ref[i].matchnum],
                   end_i = ref[i].start + len_i;
    for (j = i + 1; j < 2 * n; j++)
    {
      uint64_t val = 0;
      int cls;
      if (vsa_mc_stops(&mc, end_i, ref[j].start))
      {
        break;
      }
      st.candidates++;
      cls = vsa_mc_classify(&mc, end_i, len_i, ref[i].matchnum, ref[j].start,
                            length[ref[j].matchnum], ref[j].matchnum, &val);
      if (cls == VSA_MC_SAME)
      {
        st.samematch++;
      } else if (cls == VSA_MC_BELOW)
      {
        st.below++;
      } else
      {
        if (e.n + 1 >= 0xFFFFFFFFull)
        {
          rc = vsa_fail(VSA_NOT_COVERED, "%s: only fewer than 2^32 - 1 edges "
                        "are covered", who);
          goto done;
        }
        if (addedge(&e, ref[i].matchnum, ref[j].matchnum, val) != 0)
        {
          rc = -1;
          goto done;
        }
      }
    }
  }
  rc = deliver(who, n, &e, &st, stats, clusterstart,
               members, label, edgestart, m0, m1, value, edgecapacity, buffer,
               capacity, written);
done:
  free(e.m0);
  free(e.m1);
  free(e.value);
  free(ref);
  free(tmp);
  free(length);
  return rc;
}

/* ---- erate: uedistcluster, Vmatch/cluedist.c:120-198 ----------------------- */

int vsa_er_checklayout(const vsa_sinkparams *layout, uint32_t errorrate,
                       uint64_t textlength, const char *who,
                       vsa_selrules *rules)
{
  if (layout == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (errorrate > 100)
  {
    return vsa_fail(-2, "%s: an error rate of %lu is beyond 100", who,
                    (unsigned long) errorrate);
  }
  if (vsa_layout_selfpalindromic(layout, who) != 0)
  {
    return VSA_NOT_COVERED;
  }
  if (layout->kind != VSA_SINK_SELF || layout->totalquerylength > 0)
  {
    /* (the reference takes them and reads position2 off the index text) */
    return vsa_fail(VSA_NOT_COVERED, "%s: matchcluster erate covers lists of "
                    "an index against itself only: the second instance of a "
                    "match against queries is no stretch of the index text",
                    who);
  }
  if (layout->totallength == 0 || layout->totallength != textlength)
  {
    return vsa_fail(-2, "%s: a layout of %lu symbols, a text of %lu", who,
                    (unsigned long) layout->totallength,
                    (unsigned long) textlength);
  }
  /* a self layout without indexed queries: none of the shared refusals */
  return vsa_layout_view(layout, who, 0, rules);
}

/* verifysmalldistance and unitedistfrontSEPgeneric with a bound
   (cluedist.c:42-106, frontSEP.c:341-446) through the rules; front: 2 *
   (2 * maxdist + 3) words */
static int64_t instancepair(const uint8_t *text, uint64_t pu, uint64_t ulen,
                            uint64_t pv, uint64_t vlen, uint64_t maxdist,
                            int64_t *front)
{
  const int64_t goal = (int64_t) vlen - (int64_t) ulen,
                md = (int64_t) maxdist;
  /* prev[k] and cur[k] for k = -md - 1 .. md + 1 */
  int64_t *prev = front + md + 1, *cur = front + 3 * md + 4, *swap;
  int64_t d, k;

  if (vsa_er_lengthfails(ulen, vlen, maxdist))
  {
    return -1;
  }
  if (vsa_er_sameinstance(pu, ulen, pv, vlen))
  {
    return 0;
  }
  for (k = -md - 1; k <= md + 1; k++)
  {
    prev[k] = cur[k] = VSA_ER_NEG;
  }
  prev[0] = vsa_er_slide(text, pu, ulen, pv, vlen, 0, 0);
  if (goal == 0 && prev[0] == (int64_t) ulen)
  {
    return 0;
  }
  for (d = 1; d <= md; d++)
  {
    for (k = -d; k <= d; k++)
    {
      cur[k] = vsa_er_entry(text, pu, ulen, pv, vlen,
                            vsa_er_best(prev[k], prev[k - 1], prev[k + 1]),
                            k);
    }
    if (-d <= goal && goal <= d && cur[goal] == (int64_t) ulen)
    {
      return d;
    }
    swap = prev;
    prev = cur;
    cur = swap;
  }
  return -1;
}

int vsa_eratecluster_host(const vsa_sinkparams *layout, uint32_t errorrate,
                          const uint8_t *text, uint64_t textlength,
                          const vsa_match *matches, uint64_t n,
                          vsa_matchclusterstats *stats, uint64_t *clusterstart,
                          uint64_t *members, uint64_t *label,
                          uint64_t *edgestart, uint32_t *m0, uint32_t *m1,
                          uint64_t *value, uint64_t edgecapacity, char *buffer,
                          uint64_t capacity, int64_t *written)
{
  static const char who[] = "vsa_eratecluster_host";
  vsa_selrules rules;
  vsa_matchclusterstats st;
  Edges e = {NULL, NULL, NULL, 0, 0};
  uint64_t *length = NULL, *pos = NULL;
  int64_t *front = NULL;
  uint64_t i, j, longest = 0;
  int rc = vsa_er_checklayout(layout, errorrate, textlength, who, &rules);

  if (rc != 0)
  {
    return rc;
  }
  if (text == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if ((rc = vsa_list_check(who, "matches", matches, n)) != 0)
  {
    return rc;
  }
  memset(&st, 0, sizeof st);
  st.matches = n;
  length = malloc((size_t) (n + 1) * sizeof *length);
  pos = malloc((size_t) (2 * n + 1) * sizeof *pos);
  if (length == NULL || pos == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  for (i = 0; i < n; i++)
  {
    vsa_selvalues v;
    if (vsa_sel_values(&rules, matches + i, 0, &v) != 0)
    {
      rc = -2;
    } else
    {
      rc = vsa_er_checkrecord(text, textlength, v.length1, v.position1,
                              v.position2);
    }
    if (rc != 0)
    {
      vsa_fail(rc, rc == -2
               ? "%s: record %lu does not fit the layout (it leaves the text "
                 "or holds a separator)"
               : "%s: record %lu: only lengths below 2^32 are covered", who,
               (unsigned long) i);
      goto done;
    }
    length[i] = v.length1;
    pos[2 * i] = v.position1;
    pos[2 * i + 1] = v.position2;
    if (longest < v.length1)
    {
      longest = v.length1;
    }
  }
  front = malloc((size_t) (4 * vsa_er_maxdist(longest, errorrate) + 8) *
                 sizeof *front);
  if (front == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  for (i = 0; i + 1 < n; i++)
  {
    for (j = i + 1; j < n; j++)
    {
      const uint64_t minlen = length[i] < length[j] ? length[i] : length[j],
                     maxdist = vsa_er_maxdist(minlen, errorrate);
      int64_t edist = -1;
      int c;
      st.candidates++;
      for (c = 0; c < 4 && edist < 0; c++)
      {
        edist = instancepair(text, pos[2 * i + vsa_er_first(c)], length[i],
                             pos[2 * j + vsa_er_second(c)], length[j],
                             maxdist, front);
      }
      if (edist < 0)
      {
        st.below++;
        continue;
      }
      if (e.n + 1 >= 0xFFFFFFFFull)
      {
        rc = vsa_fail(VSA_NOT_COVERED, "%s: only fewer than 2^32 - 1 edges "
                      "are covered", who);
        goto done;
      }
      if (addedge(&e, (uint32_t) i, (uint32_t) j,
                  vsa_er_value(minlen, (uint64_t) edist)) != 0)
      {
        rc = -1;
        goto done;
      }
    }
  }
  rc = deliver(who, n, &e, &st, stats, clusterstart, members, label,
               edgestart, m0, m1, value, edgecapacity, buffer, capacity,
               written);
done:
  free(e.m0);
  free(e.m1);
  free(e.value);
  free(length);
  free(pos);
  free(front);
  return rc;
}
