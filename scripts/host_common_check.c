/*
  vstree_amd/csrc/host_common.h as a program of its own, for runs under a
  sanitizer (tests/test_host_common.py builds it with
  -fsanitize=address,undefined together with chain_host.c,
  matchcluster_host.c, cluster_host.c, select_host.c and match_sink.c).  No
  GPU, no Python in the process.

  It drives the message buffer with a name longer than the buffer, the text
  buffer at capacity 0, one byte short and exact, the layout view over every
  defect a layout can have, and one list on the layout of
  tests/golden/micro_db.fna through vsa_chain_host, vsa_matchcluster_host and
  vsa_select_host with their formatters, every buffer on the heap and of the
  exact size.  The last line is "host_common_check: ok"; the first thing
  that is not as expected ends the program with 1.
*/
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include "vstree_amd.h"
#include "host_common.h"

/* on the heap and of the exact size: one byte too many is seen */
static char *errbuf;

char *vsa_errbuf(void)
{
  return errbuf;
}

#define EXPECT(COND)                                                          \
  do                                                                          \
  {                                                                           \
    if (!(COND))                                                              \
    {                                                                         \
      fprintf(stderr, "%s:%d: %s fails; message \"%s\"\n", __FILE__,          \
              __LINE__, #COND, errbuf);                                       \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

static void messagebuffer(void)
{
  char *who = malloc(3 * VSA_ERRBUF_SIZE + 1);

  EXPECT(who != NULL);
  memset(who, 'w', 3 * VSA_ERRBUF_SIZE);
  who[3 * VSA_ERRBUF_SIZE] = '\0';
  EXPECT(vsa_fail(-7, "%s: incomplete layout", who) == -7);
  EXPECT(strlen(errbuf) == VSA_ERRBUF_SIZE - 1);
  EXPECT(errbuf[0] == 'w' && errbuf[VSA_ERRBUF_SIZE - 2] == 'w');
  EXPECT(vsa_list_misfit(who, 3) == -2);
  EXPECT(strlen(errbuf) == VSA_ERRBUF_SIZE - 1);
  EXPECT(vsa_fail(5, "%s %d", "short", 1) == 5);
  EXPECT(strcmp(errbuf, "short 1") == 0);
  free(who);
}

/* "abc\n" and "de 7\n" into a buffer of cap bytes -> what vsa_endtext says */
static int64_t ninebytes(char *p, uint64_t cap)
{
  vsa_textbuf t = {p, cap, 0};

  vsa_put(&t, "abc\n", 4);
  vsa_putf(&t, "de %d\n", 7);
  return vsa_endtext(&t, "ninebytes");
}

static void textbuffer(void)
{
  uint64_t cap;

  for (cap = 0; cap <= 12; cap++)
  {
    /* (no buffer of 0 bytes: malloc(0) may be NULL) */
    char *p = malloc(cap ? cap : 1);
    char want[64];
    int64_t n;

    EXPECT(p != NULL);
    memset(p, 'U', cap ? cap : 1);
    n = ninebytes(p, cap);
    if (cap <= 9)
    {
      snprintf(want, sizeof want, "ninebytes: 10 bytes do not fit a buffer "
               "of %lu", (unsigned long) cap);
      EXPECT(n == -3 && strcmp(errbuf, want) == 0);
      /* the first line where it fits with room to spare, nothing else */
      EXPECT(memcmp(p, cap > 4 ? "abc\nUUUUU" : "UUUUUUUUU", cap) == 0);
      EXPECT(cap != 0 || p[0] == 'U');
    } else
    {
      EXPECT(n == 9 && memcmp(p, "abc\nde 7\n", 10) == 0);
      EXPECT(cap < 11 || p[10] == 'U');
    }
    free(p);
  }
  {
    /* a line of 600 bytes is cut at 511, not read beyond its buffer */
    char *p = malloc(1024), big[601];
    vsa_textbuf t = {p, 1024, 0};
    memset(big, 'x', 600);
    big[600] = '\0';
    vsa_putf(&t, "%s", big);
    EXPECT(vsa_endtext(&t, "long") == 511 && strlen(p) == 511);
    free(p);
  }
}

/* ---- the layout of tests/golden/micro_db.fna ------------------------------ */

static const uint64_t markpos[2] = {31, 50}, qstart[3] = {0, 32, 51},
                      qlen[3] = {31, 18, 12};

static vsa_sinkparams microlayout(int kind)
{
  vsa_sinkparams l;

  memset(&l, 0, sizeof l);
  l.kind = kind;
  l.numofchars = 4;
  l.totallength = 63;
  l.numofsequences = 3;
  l.markpos = markpos;
  if (kind != VSA_SINK_SELF)
  {
    l.numofqueries = 3;
    l.querytotallength = 63;
    l.querystart = qstart;
    l.querylength = qlen;
  }
  return l;
}

#define ALLNEEDS                                                              \
  (VSA_NEEDS_NOSELFPAL | VSA_NEEDS_SEQUENCES | VSA_NEEDS_QUERIES |            \
   VSA_NEEDS_CHARS)

/* the view under `needs` answers rc with the message, and with every need
   asked for allrc with the same message, or the selfpalindromic one for such
   a layout */
static void view(const vsa_sinkparams *l, int needs, int rc, int allrc,
                 const char *message)
{
  static const char selfpal[] = "w: lists of vmatch -p IDX (selfpalindromic) "
                                "are not covered";
  vsa_selrules v;

  memset(&v, 0x55, sizeof v);
  EXPECT(vsa_layout_view(l, "w", needs, &v) == rc);
  if (rc != 0)
  {
    EXPECT(strcmp(errbuf, message != NULL ? message : selfpal) == 0);
    EXPECT(v.kind == 0x55555555); /* untouched */
  } else
  {
    EXPECT(v.kind == l->kind && v.noevalue == 1 && v.table == NULL &&
           v.totallength == (double) l->totallength);
    EXPECT(l->kind == VSA_SINK_SELF
               ? v.nq == 0 && v.qstart == NULL &&
                     v.dblenplus1 == l->totallength - l->totalquerylength &&
                     v.hasindexedqueries == (l->totalquerylength > 0)
               : v.nq == l->numofqueries && v.qstart == l->querystart &&
                     v.qlen == l->querylength && v.dblenplus1 == 0);
  }
  EXPECT(vsa_layout_view(l, "w", ALLNEEDS, &v) == allrc);
  EXPECT(allrc == 0 ||
         strcmp(errbuf, l->selfpalindromic ? selfpal : message) == 0);
}

static void layoutview(void)
{
  static const char translated[] = "w: lists of a six-frame translated batch "
                                   "(VSA_SINK_TRANSLATED) are not covered",
                    incomplete[] = "w: incomplete layout";
  vsa_sinkparams l;
  int kind;

  for (kind = VSA_SINK_COMPLETE; kind <= VSA_SINK_APPROX_HAMMING; kind++)
  {
    l = microlayout(kind);
    view(&l, 0, 0, 0, NULL);
  }
  for (kind = VSA_SINK_TRANSLATED; kind <= VSA_SINK_TRANSLATED_COMPLETE;
       kind++)
  {
    l = microlayout(kind);
    view(&l, 0, VSA_NOT_COVERED, VSA_NOT_COVERED, translated);
    l.totallength = 0; /* the translated refusal comes first */
    view(&l, 0, VSA_NOT_COVERED, VSA_NOT_COVERED, translated);
    l.selfpalindromic = 1; /* ... and the selfpalindromic one before it */
    view(&l, VSA_NEEDS_NOSELFPAL, VSA_NOT_COVERED, VSA_NOT_COVERED, NULL);
    view(&l, ALLNEEDS & ~VSA_NEEDS_NOSELFPAL, VSA_NOT_COVERED,
         VSA_NOT_COVERED, translated);
  }
  l = microlayout(VSA_SINK_QUERY);
  l.selfpalindromic = 1;
  view(&l, 0, 0, VSA_NOT_COVERED, NULL);
  l = microlayout(VSA_SINK_SELF);
  l.totallength = 0;
  view(&l, 0, -2, -2, incomplete);
  l = microlayout(VSA_SINK_SELF);
  l.totalquerylength = 63;
  view(&l, 0, -2, -2, incomplete);
  l.totalquerylength = 62; /* an index of queries alone, but a layout */
  view(&l, 0, 0, 0, NULL);
  l = microlayout(VSA_SINK_SELF);
  l.numofsequences = 2;
  l.markpos = NULL;
  view(&l, ALLNEEDS & ~VSA_NEEDS_SEQUENCES, 0, -2, incomplete);
  l.numofsequences = 1; /* one sequence has no separator */
  view(&l, ALLNEEDS, 0, 0, NULL);
  l.numofsequences = 0;
  view(&l, ALLNEEDS & ~VSA_NEEDS_SEQUENCES, 0, -2, incomplete);
  l = microlayout(VSA_SINK_QUERY);
  l.querystart = NULL;
  view(&l, ALLNEEDS & ~VSA_NEEDS_QUERIES, 0, -2, incomplete);
  l = microlayout(VSA_SINK_QUERY);
  l.querylength = NULL;
  view(&l, ALLNEEDS & ~VSA_NEEDS_QUERIES, 0, -2, incomplete);
  l.numofqueries = 0; /* no queries, no arrays */
  view(&l, ALLNEEDS, 0, 0, NULL);
  l = microlayout(VSA_SINK_SELF);
  l.querystart = l.querylength = NULL; /* a self layout has none */
  l.numofqueries = 3;
  view(&l, ALLNEEDS, 0, 0, NULL);
  l = microlayout(VSA_SINK_SELF);
  l.numofchars = 1;
  view(&l, ALLNEEDS & ~VSA_NEEDS_CHARS, 0, -2, incomplete);
  for (kind = -1; kind <= 7; kind += 8)
  {
    l = microlayout(VSA_SINK_SELF);
    l.kind = kind;
    view(&l, 0, -2, -2, incomplete);
  }
}

static void lists(void)
{
  vsa_match rec[3] = {{8, 0, 15, 0}, {8, 0, 38, 0}, {8, 15, 55, 0}};
  const uint8_t flags[3] = {0, 1, 0};
  int pal = 7;

  EXPECT(vsa_list_check("w", "records", NULL, 0) == 0);
  EXPECT(vsa_list_check("w", "records", NULL, 1) == -1 &&
         strcmp(errbuf, "w: NULL argument") == 0);
  EXPECT(vsa_list_check("w", "records", rec, 0xFFFFFFFFull) ==
             VSA_NOT_COVERED &&
         strcmp(errbuf, "w: 4294967295 records: only fewer than 2^32 - 1 are "
                        "covered") == 0);
  EXPECT(vsa_list_check("w", "records", rec, 0xFFFFFFFEull) == 0);
  EXPECT(vsa_list_check("w", NULL, rec, 0xFFFFFFFFull) == 0);
  EXPECT(vsa_list_flag("w", VSA_SINK_SELF, NULL, 1, &pal) == 0 && pal == 0);
  EXPECT(vsa_list_flag("w", VSA_SINK_QUERY, flags, 1, &pal) == 0 && pal == 1);
  EXPECT(vsa_list_flag("w", VSA_SINK_SELF, flags, 2, &pal) == 0 && pal == 0);
  EXPECT(vsa_list_flag("w", VSA_SINK_SELF, flags, 1, &pal) ==
             VSA_NOT_COVERED &&
         strcmp(errbuf, "w: palindromic self matches are the selfpalindromic "
                        "form") == 0);
}

/* the text fmt(buffer, capacity, info) writes, into buffers of the exact
   sizes around its length -> the text, owned by the caller */
static char *exact(int64_t (*fmt)(char *, uint64_t, void *), void *info)
{
  char *big = malloc(4096), *p;
  const int64_t n = fmt(big, 4096, info);
  int64_t cap;

  EXPECT(n > 0 && n < 4095 && (int64_t) strlen(big) == n);
  for (cap = 0; cap <= n + 1; cap += cap == 1 && n > 2 ? n - 2 : 1)
  {
    p = malloc(cap ? (size_t) cap : 1);
    if (cap <= n)
    {
      EXPECT(fmt(p, (uint64_t) cap, info) == -3);
    } else
    {
      EXPECT(fmt(p, (uint64_t) cap, info) == n && memcmp(p, big, n + 1) == 0);
    }
    free(p);
  }
  return big;
}

typedef struct
{
  vsa_sink *sink;
  const vsa_sinkparams *layout;
  const vsa_match *rec;
  uint64_t nchains, *number, *start, *members;
  int64_t *score;
  vsa_match *chained;
} Microlist;

static int64_t chaintext(char *buffer, uint64_t capacity, void *info)
{
  const Microlist *m = info;
  return vsa_chain_format_host(m->sink, 0, m->nchains, m->number, m->score,
                               m->start, m->chained, buffer, capacity);
}

static int64_t clustertext(char *buffer, uint64_t capacity, void *info)
{
  const Microlist *m = info;
  const vsa_matchclusterparams p = {VSA_MATCHCLUSTER_GAP, 7, 0};
  int64_t written = 0;
  const int rc = vsa_matchcluster_host(m->layout, &p, m->rec, NULL, 3, NULL,
                                       NULL, NULL, NULL, NULL, NULL, NULL,
                                       NULL, 0, buffer, capacity, &written);
  return rc == 0 ? written : rc;
}

static int64_t clusterfile(char *buffer, uint64_t capacity, void *info)
{
  const Microlist *m = info;
  const uint64_t member[3] = {0, 2, 1}, value[2] = {0, 7};
  const uint32_t m0[2] = {0, 0}, m1[2] = {1, 2};
  return vsa_matchcluster_format_host(m->sink, VSA_MATCHCLUSTER_GAP, member,
                                      m->rec, 3, m0, m1, value, 2, buffer,
                                      capacity);
}

static void microlist(void)
{
  const vsa_sinkparams layout = microlayout(VSA_SINK_SELF);
  const vsa_match rec[3] = {{8, 0, 15, 0}, {8, 0, 38, 0}, {8, 15, 55, 0}};
  vsa_chainparams cp;
  vsa_selectparams sp;
  vsa_chainstats st;
  vsa_match *selected = malloc(3 * sizeof *selected);
  uint64_t nselected = 0, i;
  Microlist m;
  char *text;

  memset(&m, 0, sizeof m);
  m.layout = &layout;
  m.rec = rec;
  EXPECT(vsa_sink_open(&layout, &m.sink) == 0);
  /* chains over the whole list, in arrays of the sizes the first call says */
  memset(&cp, 0, sizeof cp);
  cp.kind = VSA_CHAIN_GLOBAL;
  cp.weightfactor = 1.0;
  EXPECT(vsa_chain_host(&layout, &cp, rec, NULL, 3, &st, NULL, NULL, NULL,
                        NULL, 0, NULL, 0) == 0);
  EXPECT(st.matches == 3 && st.chains >= 1 && st.chained >= st.chains &&
         st.chained <= 3);
  m.nchains = st.chains;
  m.number = malloc((size_t) st.chains * sizeof *m.number);
  m.score = malloc((size_t) st.chains * sizeof *m.score);
  m.start = malloc((size_t) (st.chains + 1) * sizeof *m.start);
  m.members = malloc((size_t) st.chained * sizeof *m.members);
  m.chained = malloc((size_t) st.chained * sizeof *m.chained);
  EXPECT(vsa_chain_host(&layout, &cp, rec, NULL, 3, NULL, NULL, m.number,
                        m.score, m.start, st.chains, m.members,
                        st.chained - 1) == -3);
  EXPECT(vsa_chain_host(&layout, &cp, rec, NULL, 3, NULL, NULL, m.number,
                        m.score, m.start, st.chains, m.members,
                        st.chained) == 0);
  EXPECT(m.start[0] == 0 && m.start[st.chains] == st.chained);
  for (i = 0; i < st.chained; i++)
  {
    EXPECT(m.members[i] < 3);
    m.chained[i] = rec[m.members[i]];
  }
  text = exact(chaintext, &m);
  EXPECT(strncmp(text, "# chain 0: length ", 18) == 0);
  fputs(text, stdout);
  free(text);
  text = exact(clustertext, &m);
  EXPECT(strcmp(text, "# cluster 3 matches\n# create cluster 0 of size 3\n")
         == 0);
  fputs(text, stdout);
  free(text);
  text = exact(clusterfile, &m);
  EXPECT(strncmp(text, "# id 0\n", 7) == 0 &&
         strstr(text, "# linked 0 and 2 with gapsize 7\n") != NULL);
  fputs(text, stdout);
  free(text);
  /* the selection of everything, and of nothing under a translated layout */
  memset(&sp, 0, sizeof sp);
  sp.sortmode = VSA_SORT_NONE;
  EXPECT(vsa_select_host(&layout, &sp, rec, NULL, 3, selected, NULL, NULL, 3,
                         &nselected, NULL) == 0 && nselected == 3);
  EXPECT(vsa_select_host(&layout, &sp, rec, NULL, 3, selected, NULL, NULL, 2,
                         &nselected, NULL) == -3);
  {
    vsa_sinkparams t = layout;
    t.kind = VSA_SINK_TRANSLATED;
    EXPECT(vsa_select_host(&t, &sp, rec, NULL, 3, selected, NULL, NULL, 3,
                           &nselected, NULL) == VSA_NOT_COVERED);
    EXPECT(strcmp(errbuf, "vsa_select: lists of a six-frame translated batch "
                          "(VSA_SINK_TRANSLATED) are not covered") == 0);
    EXPECT(vsa_chain_host(&t, &cp, rec, NULL, 3, NULL, NULL, NULL, NULL, NULL,
                          0, NULL, 0) == VSA_NOT_COVERED);
  }
  vsa_sink_close(m.sink);
  free(m.number);
  free(m.score);
  free(m.start);
  free(m.members);
  free(m.chained);
  free(selected);
}

int main(void)
{
  errbuf = malloc(VSA_ERRBUF_SIZE);
  if (errbuf == NULL)
  {
    return 2;
  }
  errbuf[0] = '\0';
  messagebuffer();
  textbuffer();
  layoutview();
  lists();
  microlist();
  free(errbuf);
  printf("host_common_check: ok\n");
  return 0;
}
