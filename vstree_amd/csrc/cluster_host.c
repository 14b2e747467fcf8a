/*
  Sequence clustering, host side: a fresh restatement of the reference's
  ClusterSet (kurtz/cluster.c:401-578: makenewcluster, appendcluster,
  linkmulticluster, linkcluster), the numbering and member order of
  showClusterSet (cluster.c:125-197), the lines of clusterSizedistribution
  (cluster.c:638-683) and of processvmcluster (Vmatch/vmcluster.c:19-72,
  417-432), and vsa_cluster_host, which sends every accepted record of a list
  in host memory through linkcluster.  cluster.hip sends only the edges of
  the spanning forest it found through the same code.  No GPU involved.
*/
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "cluster_rules.h"
#include "host_common.h"

#define NIL 0xFFFFFFFFu

typedef struct
{
  uint64_t numofelems, nclusters;
  uint32_t *cnum, *next; /* per element; cnum == NIL: in no cluster         */
  uint64_t *csize;       /* per cluster, in the order of creation           */
  uint32_t *first, *last;
} clset;

static void clset_free(clset *s)
{
  free(s->cnum);
  free(s->next);
  free(s->csize);
  free(s->first);
  free(s->last);
  memset(s, 0, sizeof *s);
}

static int clset_init(clset *s, uint64_t numofelems)
{
  /* every new cluster takes two elements out of the singletons */
  const size_t maxclusters = (size_t) (numofelems / 2 + 1);

  memset(s, 0, sizeof *s);
  s->numofelems = numofelems;
  s->cnum = malloc((size_t) numofelems * sizeof *s->cnum);
  s->next = malloc((size_t) numofelems * sizeof *s->next);
  s->csize = malloc(maxclusters * sizeof *s->csize);
  s->first = malloc(maxclusters * sizeof *s->first);
  s->last = malloc(maxclusters * sizeof *s->last);
  if (s->cnum == NULL || s->next == NULL || s->csize == NULL ||
      s->first == NULL || s->last == NULL)
  {
    clset_free(s);
    return vsa_fail(-1, "out of memory");
  }
  memset(s->cnum, 0xFF, (size_t) numofelems * sizeof *s->cnum);
  return 0;
}

static void clset_append(clset *s, uint32_t c, uint32_t elem)
{
  s->cnum[elem] = c;
  s->next[elem] = NIL;
  s->next[s->last[c]] = elem;
  s->last[c] = elem;
  s->csize[c]++;
}

/* linkcluster; 1 if the edge joined two different clusters, else 0 */
static int clset_link(clset *s, uint32_t e1, uint32_t e2)
{
  uint32_t c1 = s->cnum[e1], c2 = s->cnum[e2], target, source, i;

  if (c1 == NIL && c2 == NIL)
  {
    const uint32_t c = (uint32_t) s->nclusters++;
    s->cnum[e1] = s->cnum[e2] = c;
    s->next[e1] = e2;
    s->next[e2] = NIL;
    s->csize[c] = 2;
    s->first[c] = e1;
    s->last[c] = e2;
    return 1;
  }
  if (c1 == NIL)
  {
    clset_append(s, c2, e1);
    return 1;
  }
  if (c2 == NIL)
  {
    clset_append(s, c1, e2);
    return 1;
  }
  if (c1 == c2)
  {
    return 0;
  }
  /* the larger cluster is the target; of two equally large ones that of
     the second element (cluster.c:564-572) */
  if (s->csize[c1] > s->csize[c2])
  {
    target = c1;
    source = c2;
  } else
  {
    source = c1;
    target = c2;
  }
  for (i = s->first[source]; i != NIL; i = s->next[i])
  {
    s->cnum[i] = target;
  }
  s->next[s->last[target]] = s->first[source];
  s->first[source] = NIL;
  s->last[target] = s->last[source];
  s->csize[target] += s->csize[source];
  s->csize[source] = 0;
  return 1;
}

void vsa_cl_freeresult(vsa_clresult *r)
{
  free(r->clusterstart);
  free(r->members);
  free(r->label);
  memset(r, 0, sizeof *r);
}

/* the numbering of showClusterSet: clusters in the order of creation, the
   emptied ones left out; the members along the chain */
static int clset_result(const clset *s, vsa_clresult *r)
{
  uint64_t c, k = 0, pos = 0, in = 0, e;
  uint32_t i;

  memset(r, 0, sizeof *r);
  for (c = 0; c < s->nclusters; c++)
  {
    if (s->csize[c] > 0)
    {
      k++;
      in += s->csize[c];
    }
  }
  r->numofsequences = s->numofelems;
  r->clusters = k;
  r->inclusters = in;
  r->clusterstart = malloc((size_t) (k + 1) * sizeof *r->clusterstart);
  r->members = malloc((size_t) (in + 1) * sizeof *r->members);
  r->label = malloc((size_t) (s->numofelems + 1) * sizeof *r->label);
  if (r->clusterstart == NULL || r->members == NULL || r->label == NULL)
  {
    vsa_cl_freeresult(r);
    return vsa_fail(-1, "out of memory");
  }
  for (e = 0; e < s->numofelems; e++)
  {
    r->label[e] = VSA_CLUSTER_SINGLET;
  }
  k = 0;
  for (c = 0; c < s->nclusters; c++)
  {
    if (s->csize[c] == 0)
    {
      continue;
    }
    r->clusterstart[k] = pos;
    for (i = s->first[c]; i != NIL; i = s->next[i])
    {
      r->members[pos++] = i;
      r->label[i] = k;
    }
    if (pos - r->clusterstart[k] != s->csize[c])
    {
      vsa_cl_freeresult(r);
      return vsa_fail(-101, "vsa_cluster: the chain of cluster %lu does not "
                      "have its %lu elements", (unsigned long) k,
                      (unsigned long) s->csize[c]);
    }
    k++;
  }
  r->clusterstart[k] = pos;
  return 0;
}

int vsa_cl_replay(uint64_t numofsequences, const uint32_t *e1,
                  const uint32_t *e2, uint64_t nedges, uint64_t *changed,
                  vsa_clresult *result)
{
  clset s;
  uint64_t i, ch = 0;
  int rc;

  memset(result, 0, sizeof *result);
  if (clset_init(&s, numofsequences) != 0)
  {
    return -1;
  }
  for (i = 0; i < nedges; i++)
  {
    if (e1[i] >= numofsequences || e2[i] >= numofsequences || e1[i] == e2[i])
    {
      clset_free(&s);
      return vsa_fail(-101, "vsa_cluster: edge %lu (%lu, %lu) among %lu "
                      "sequences", (unsigned long) i, (unsigned long) e1[i],
                      (unsigned long) e2[i], (unsigned long) numofsequences);
    }
    ch += (uint64_t) clset_link(&s, e1[i], e2[i]);
  }
  rc = clset_result(&s, result);
  clset_free(&s);
  if (changed != NULL)
  {
    *changed = ch;
  }
  return rc;
}

int64_t vsa_cl_format(const vsa_clresult *r, char *buffer, uint64_t capacity)
{
  vsa_textbuf t = {buffer, capacity, 0};
  const uint64_t all = r->numofsequences, in = r->inclusters;
  uint64_t *dist, c, i;

  dist = calloc((size_t) all + 1, sizeof *dist);
  if (dist == NULL)
  {
    return vsa_fail(-1, "out of memory");
  }
  for (c = 0; c < r->clusters; c++)
  {
    dist[r->clusterstart[c + 1] - r->clusterstart[c]]++;
  }
  vsa_putf(&t, "# %lu cluster%s\n", (unsigned long) r->clusters,
           r->clusters == 1 ? "" : "s");
  vsa_putf(&t, "# %lu elements out of %lu (%.2f%%) are in clusters\n",
           (unsigned long) in, (unsigned long) all, 100.0 * (double) in / all);
  vsa_putf(&t, "# %lu elements out of %lu (%.2f%%) are singlets\n",
           (unsigned long) (all - in), (unsigned long) all,
           100.0 * (double) (all - in) / all);
  for (i = 2; i <= all; i++)
  {
    if (dist[i] > 0)
    {
      vsa_putf(&t, "# %lu cluster%s of size %lu\n", (unsigned long) dist[i],
               dist[i] > 1 ? "s" : "", (unsigned long) i);
    }
  }
  free(dist);
  for (c = 0; c < r->clusters; c++)
  {
    vsa_putf(&t, "%lu: ", (unsigned long) c);
    for (i = r->clusterstart[c]; i < r->clusterstart[c + 1]; i++)
    {
      vsa_putf(&t, " %lu", (unsigned long) r->members[i]);
    }
    vsa_put(&t, "\n", 1);
  }
  return vsa_endtext(&t, "vsa_cluster_format");
}

int vsa_cl_checklayout(const vsa_sinkparams *layout,
                       const vsa_clusterparams *params, const char *who)
{
  if (layout == NULL || params == NULL)
  {
    return vsa_fail(-1, "%s: NULL argument", who);
  }
  if (layout->kind != VSA_SINK_SELF &&
      !(layout->kind == VSA_SINK_QUERY && layout->selfpalindromic))
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: only self lists and lists of "
                    "vmatch -p IDX are covered, not layout kind %d", who,
                    layout->kind);
  }
  if (layout->numofsequences == 1)
  {
    return vsa_fail(-2, "option -dbcluster only possible for index with at "
                    "least two sequences");
  }
  if (layout->numofquerysequences > 0)
  {
    return vsa_fail(-2, "option -dbcluster requires index without query "
                    "sequences");
  }
  if (layout->numofsequences >= 0xFFFFFFFFull)
  {
    return vsa_fail(VSA_NOT_COVERED, "%s: %lu sequences: only fewer than "
                    "2^32 - 1 are covered", who,
                    (unsigned long) layout->numofsequences);
  }
  if (layout->numofsequences == 0 || layout->markpos == NULL)
  {
    return vsa_fail(-2, "%s: incomplete layout", who);
  }
  return 0;
}

int vsa_cluster_host(const vsa_sinkparams *layout,
                     const vsa_clusterparams *params, const vsa_match *matches,
                     const uint8_t *palindromic, uint64_t n,
                     vsa_clusterstats *stats, uint64_t *clusterstart,
                     uint64_t *members, uint64_t *label, uint64_t *edgestart,
                     uint64_t *edgerecord, char *buffer, uint64_t capacity,
                     int64_t *written)
{
  static const char who[] = "vsa_cluster_host";
  vsa_clrules rules;
  vsa_clusterstats st;
  vsa_clresult res;
  uint32_t *e1 = NULL, *e2 = NULL;
  uint64_t *rec = NULL, *fill = NULL;
  uint64_t i, m = 0, count[VSA_CL_CLASSES] = {0};
  int64_t bytes = 0;
  int rc = vsa_cl_checklayout(layout, params, who);

  /* (any number of records: the sequences are what is counted in 32 bits) */
  if (rc != 0 || (rc = vsa_list_check(who, NULL, matches, n)) != 0)
  {
    return rc;
  }
  rules.totallength = layout->totallength;
  rules.numofsequences = layout->numofsequences;
  rules.markpos = layout->markpos;
  rules.percsmall = params->percsmall;
  rules.perclarge = params->perclarge;
  e1 = malloc((size_t) (n + 1) * sizeof *e1);
  e2 = malloc((size_t) (n + 1) * sizeof *e2);
  rec = malloc((size_t) (n + 1) * sizeof *rec);
  if (e1 == NULL || e2 == NULL || rec == NULL)
  {
    rc = vsa_fail(-1, "out of memory");
    goto done;
  }
  for (i = 0; i < n; i++)
  {
    const int pal = palindromic != NULL && palindromic[i] != 0;
    uint64_t s1 = 0, s2 = 0;
    int cls;
    if (!pal && layout->kind != VSA_SINK_SELF)
    {
      rc = vsa_fail(VSA_NOT_COVERED, "%s: record %lu is a direct match, the "
                    "layout is that of vmatch -p IDX", who,
                    (unsigned long) i);
      goto done;
    }
    cls = vsa_cl_classify(&rules, &matches[i], pal, &s1, &s2);
    if (cls == VSA_CL_BAD)
    {
      rc = vsa_fail(-2, "%s: record %lu does not fit the layout (a match "
                    "that leaves its sequence, or a sequence number outside "
                    "the %lu of the index)", who, (unsigned long) i,
                    (unsigned long) rules.numofsequences);
      goto done;
    }
    count[cls]++;
    if (cls == VSA_CL_EDGE)
    {
      e1[m] = (uint32_t) s1;
      e2[m] = (uint32_t) s2;
      rec[m++] = i;
    }
  }
  memset(&st, 0, sizeof st);
  st.seen = n;
  st.samesequence = count[VSA_CL_SAME];
  st.mirrordropped = count[VSA_CL_MIRROR];
  st.rejected = count[VSA_CL_REJECTED];
  st.edges = m;
  if ((rc = vsa_cl_replay(rules.numofsequences, e1, e2, m, &st.forestedges,
                          &res)) != 0)
  {
    goto done;
  }
  st.clusters = res.clusters;
  st.inclusters = res.inclusters;
  st.singlets = res.numofsequences - res.inclusters;
  if (buffer != NULL &&
      (bytes = vsa_cl_format(&res, buffer, capacity)) < 0)
  {
    rc = (int) bytes;
    vsa_cl_freeresult(&res);
    goto done;
  }
  if (edgestart != NULL || edgerecord != NULL)
  {
    /* addClusterEdge (cluster.c:586-614): each cluster's part is filled
       from the back in the order of the edges */
    fill = calloc((size_t) res.clusters + 2, sizeof *fill);
    if (fill == NULL)
    {
      rc = vsa_fail(-1, "out of memory");
      vsa_cl_freeresult(&res);
      goto done;
    }
    for (i = 0; i < m; i++)
    {
      fill[res.label[e1[i]] + 1]++;
    }
    for (i = 0; i < res.clusters; i++)
    {
      fill[i + 1] += fill[i];
    }
    if (edgestart != NULL)
    {
      memcpy(edgestart, fill, (size_t) (res.clusters + 1) * sizeof *fill);
    }
    if (edgerecord != NULL)
    {
      /* fill[c + 1] = the end of cluster c: count down from there */
      for (i = 0; i < m; i++)
      {
        edgerecord[--fill[res.label[e1[i]] + 1]] = rec[i];
      }
    }
  }
  if (stats != NULL)
  {
    *stats = st;
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
  if (label != NULL)
  {
    memcpy(label, res.label, (size_t) res.numofsequences * sizeof *label);
  }
  if (written != NULL)
  {
    *written = bytes;
  }
  vsa_cl_freeresult(&res);
done:
  free(fill);
  free(e1);
  free(e2);
  free(rec);
  return rc;
}
