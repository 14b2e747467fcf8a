"""vstree_amd -- ctypes binding of the MI355X-native Vmengine query path.

The product is the C-ABI library vstree_amd/libvstree_amd.so (HIP kernels for
gfx950 + C host code; ABI in include/vstree_amd.h).  This module only maps it
into Python for the tests and bench.py, keeping the reference's operator names
(findcompletematches / findquerymatches / findmaximaluniquematches of
/root/reference/src/Vmengine/vmengineexport.h:4-81).

There is no CPU fallback: if the library is missing, importing fails; if no
GPU is present, every compute call returns the HIP error.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(_HERE, "libvstree_amd.so")
# same code without a link-time dependency on libamdhip64 (see csrc/Makefile)
LIBPATH_NORT = os.path.join(_HERE, "libvstree_amd_nort.so")


def _loaded_hip_runtime():
    """path of a libamdhip64 already mapped into this process, if any (e.g.
    the one a PyTorch wheel bundles under torch/lib)"""
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    return line.split()[-1]
    except OSError:
        pass
    return None

OWN_HIP_RUNTIME = "/opt/rocm/lib/libamdhip64.so"

SEPARATOR = 255
WILDCARD = 254
NO_SUBST = 0xFFFFFFFF

MATCH_DTYPE = np.dtype([("length", "<u8"), ("dbstart", "<u8"),
                        ("queryseq", "<u8"), ("querystart", "<u8")])
# vsa_match16: dbstart << 24 | length, queryseq << 16 | querystart
MATCH16_DTYPE = np.dtype([("dbstart_length", "<u8"),
                          ("queryseq_querystart", "<u8")])


def expand_match16(a):
    out = np.empty(len(a), MATCH_DTYPE)
    out["length"] = a["dbstart_length"] & np.uint64(0xFFFFFF)
    out["dbstart"] = a["dbstart_length"] >> np.uint64(24)
    out["queryseq"] = a["queryseq_querystart"] >> np.uint64(16)
    out["querystart"] = a["queryseq_querystart"] & np.uint64(0xFFFF)
    return out


class VsaError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("vstree_amd error %d: %s" % (code, message))
        self.code = code
        self.message = message


class Tables(C.Structure):
    _fields_ = [("totallength", C.c_uint64), ("prefixlength", C.c_uint32),
                ("numofchars", C.c_uint32), ("integersize", C.c_uint32),
                ("largelcpvalues", C.c_uint64), ("tis", C.c_void_p),
                ("suf", C.c_void_p), ("lcp", C.c_void_p),
                ("llv", C.c_void_p), ("bck", C.c_void_p),
                ("bwt", C.c_void_p), ("querysepposition", C.c_uint64),
                ("hasindexedqueries", C.c_int)]


class IndexInfo(C.Structure):
    _fields_ = [("totallength", C.c_uint64), ("numofcodes", C.c_uint64),
                ("largelcpvalues", C.c_uint64), ("device_bytes", C.c_uint64),
                ("prefixlength", C.c_uint32), ("numofchars", C.c_uint32),
                ("device_integersize", C.c_uint32), ("device", C.c_int),
                ("hasindexedqueries", C.c_int), ("hasbwt", C.c_int),
                ("deepprefix", C.c_uint32)]


class QueriesInfo(C.Structure):
    _fields_ = [("numofqueries", C.c_uint64), ("numofsymbols", C.c_uint64),
                ("minlength", C.c_uint64), ("maxlength", C.c_uint64),
                ("offset", C.c_uint64), ("device", C.c_int)]


class SinkParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("palindromic", C.c_int),
                ("selfpalindromic", C.c_int), ("showmode", C.c_uint32), ("numofchars", C.c_uint32),
                ("threads", C.c_int),
                ("leastlength", C.c_uint64), ("totallength", C.c_uint64),
                ("numofsequences", C.c_uint64), ("markpos", C.c_void_p),
                ("numofquerysequences", C.c_uint64),
                ("totalquerylength", C.c_uint64),
                ("numofqueries", C.c_uint64),
                ("querytotallength", C.c_uint64),
                ("querystart", C.c_void_p), ("querylength", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("count", C.c_uint64), ("sumlength", C.c_uint64),
                ("searches", C.c_uint64), ("candidates", C.c_uint64),
                ("search_kernel_ms", C.c_double),
                ("total_device_ms", C.c_double), ("anchor_ms", C.c_double),
                ("kernel_searches", C.c_uint64),
                ("first_kernel_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AlignStats(C.Structure):
    _fields_ = [("count", C.c_uint64), ("words", C.c_uint64),
                ("edist", C.c_uint64), ("staged", C.c_uint64),
                ("kernel_ms", C.c_double), ("total_device_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CoverageParams(C.Structure):
    _fields_ = [(k, C.c_int) for k in
                ("layout", "side", "palindromic", "selfpalindromic",
                 "complete", "markleft", "markright",
                 "markleftifdifferentsequence",
                 "markrightifdifferentsequence")]


class CoverageStats(C.Structure):
    _fields_ = [("positions", C.c_uint64), ("marked", C.c_uint64),
                ("separators", C.c_uint64), ("mark_ms", C.c_double),
                ("extract_ms", C.c_double), ("count_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SelectParams(C.Structure):
    _fields_ = [("bestnumber", C.c_uint64), ("sortmode", C.c_int),
                ("hasmaxevalue", C.c_int), ("maximumevalue", C.c_double),
                ("identity", C.c_uint32), ("hasleastscore", C.c_int),
                ("leastscore", C.c_int64), ("haslowergap", C.c_int),
                ("hasuppergap", C.c_int), ("lowergap", C.c_int64),
                ("uppergap", C.c_int64)]


class SelectStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("seen", "rejected", "duplicates", "selected",
                 "containedremoved")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ClusterParams(C.Structure):
    _fields_ = [("percsmall", C.c_uint32), ("perclarge", C.c_uint32)]


class ClusterStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("seen", "samesequence", "mirrordropped", "rejected", "edges",
                 "forestedges", "rounds", "clusters", "inclusters",
                 "singlets")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MatchClusterParams(C.Structure):
    _fields_ = [("mode", C.c_int), ("maxgapsize", C.c_uint64),
                ("minpercentoverlap", C.c_uint64)]


class MatchClusterStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("matches", "candidates", "samematch", "below", "edges",
                 "forestedges", "rounds", "clusters", "inclusters")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ChainParams(C.Structure):
    _fields_ = [("kind", C.c_int), ("value", C.c_int64),
                ("maxgapwidth", C.c_uint64), ("weightfactor", C.c_double),
                ("withinborders", C.c_int), ("thread", C.c_int)]


class ChainStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in
                ("matches", "problems", "single", "small", "wave", "group",
                 "largest", "tieruns", "replayed", "chains", "chained")]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


PROCESSMATCH = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)


def _load():
    global LIBPATH
    if not os.path.exists(LIBPATH):
        raise ImportError(
            "%s is missing: build it with `make -C vstree_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback"
            % LIBPATH)
    # One HIP runtime per process.  VSTREE_AMD_RUNTIME says which:
    #   own   libvstree_amd.so, which links /opt/rocm/lib/libamdhip64.so
    #   host  libvstree_amd_nort.so: the same objects, bound to the runtime the
    #         process has mapped already (a PyTorch wheel's, under torch/lib)
    #   auto  (default) host if a runtime is mapped at import time, own if not
    # -- the explicit values are for callers that do not want the outcome to
    # depend on the order of their imports: each fails where it cannot hold.
    choice = os.environ.get("VSTREE_AMD_RUNTIME", "auto")
    if choice not in ("auto", "own", "host"):
        raise ImportError("VSTREE_AMD_RUNTIME=%r: expected own, host or auto"
                          % choice)
    hip = _loaded_hip_runtime()
    if choice == "host" and hip is None:
        raise ImportError("VSTREE_AMD_RUNTIME=host, but no HIP runtime is "
                          "mapped in this process yet (import torch first)")
    if choice == "own" and hip is not None and \
            os.path.realpath(hip) != os.path.realpath(OWN_HIP_RUNTIME):
        raise ImportError("VSTREE_AMD_RUNTIME=own, but this process has "
                          "mapped %s: two HIP runtimes do not share a device"
                          % hip)
    if choice == "host" or (choice == "auto" and hip is not None and
                            os.path.exists(LIBPATH_NORT)):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)
        LIBPATH = LIBPATH_NORT
    lib = C.CDLL(LIBPATH)
    V, U64, U32, I = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    PP = C.POINTER(C.c_void_p)
    sig = {
        "vsa_messagespace": (C.c_char_p, []),
        "vsa_index_from_tables": (I, [C.POINTER(Tables), I, PP]),
        "vsa_index_open": (I, [C.c_char_p, I, PP]),
        "vsa_index_close": (None, [V]),
        "vsa_index_getinfo": (I, [V, C.POINTER(IndexInfo)]),
        "vsa_index_build": (I, [V, U64, U32, U32, I, PP]),
        "vsa_index_build_device": (I, [V, U64, U32, U32, I, PP]),
        "vsa_index_download": (I, [V, V, V, V, V, V, V]),
        "vsa_index_set_queryseparator": (I, [V, U64]),
        "vsa_index_set_queryspeedup": (I, [V, U32]),
        "vsa_index_clone": (I, [V, I, PP]),
        "vsa_pipeline_open": (I, [V, I, U64, U32, U64, PP]),
        "vsa_pipeline_hostbuffer": (V, [V]),
        "vsa_pipeline_open_packed": (I, [V, I, U64, U32, U64, U64, PP]),
        "vsa_pipeline_hostrows": (I, [V, PP, PP]),
        "vsa_pipeline_submit_packed": (I, [V, U64, U64]),
        "vsa_pipeline_submit": (I, [V, U64]),
        "vsa_pipeline_next": (I, [V, PP, C.POINTER(U64)]),
        "vsa_pipeline_finish": (I, [V, PP, C.POINTER(U64),
                                    C.POINTER(Stats)]),
        "vsa_pipeline_finish16": (I, [V, PP, C.POINTER(U64),
                                      C.POINTER(Stats)]),
        "vsa_pipeline_close": (None, [V]),
        "vsa_pipeline_set_offset": (I, [V, U64]),
        "vsa_pipeline_take_candidates": (I, [V, PP, C.POINTER(U64),
                                             C.POINTER(U32)]),
        "vsa_rows_partition_device": (I, [V, U64, U32, U32, I, U64, I, V,
                                          V]),
        "vsa_mkvtree": (I, [C.POINTER(C.c_char_p), U32, C.POINTER(C.c_char_p),
                            U32, C.c_char_p, U32, U32, I, I]),
        "vsa_queries_from_host": (I, [V, U64, V, V, U64, I, PP]),
        "vsa_queries_from_device": (I, [V, U64, U32, I, PP]),
        "vsa_packed_words": (U32, [U32]),
        "vsa_pack_reads": (I, [V, U64, U32, U64, V, V, U64, C.POINTER(U64)]),
        "vsa_pack_reads_mt": (I, [V, U64, U32, U64, V, V, U64, C.POINTER(U64),
                                  U32]),
        "vsa_queries_from_host_packed": (I, [V, U64, U32, V, U64, I, PP]),
        "vsa_queries_reverse_complement": (I, [V, PP]),
        "vsa_queries_free": (None, [V]),
        "vsa_queries_set_offset": (I, [V, U64]),
        "vsa_queries_getinfo": (I, [V, C.POINTER(QueriesInfo)]),
        "vsa_result_count": (U64, [V]),
        "vsa_result_getstats": (I, [V, C.POINTER(Stats)]),
        "vsa_result_fetch": (I, [V, V, U64]),
        "vsa_result_device_matches": (V, [V]),
        "vsa_result_free": (None, [V]),
        "vsa_result_from_host": (I, [V, U64, I, PP]),
        "vsa_result_copy_device": (I, [V, V, U64]),
        "vsa_mumuniqueinquery": (I, [V, U64, I, PP]),
        "vsa_mumuniqueinquery_range": (I, [V, U64, I, U64, PP]),
        "vsa_index_make_sti1": (I, [V, V]),
        "vsa_findcompletematches": (I, [V, V, PP]),
        "vsa_findapproxcompletematches": (I, [V, V, I, U64, I, PP]),
        "vsa_findapproxcompletematches_cb": (I, [V, V, I, U64, I,
                                                 PROCESSMATCH, V]),
        "vsa_findquerymatches": (I, [V, V, I, I, U64, PP]),
        "vsa_findmumcandidates": (I, [V, V, U64, I, PP]),
        "vsa_result_partition": (I, [V, U32, U64, V, V, V]),
        "vsa_result_partition_own": (I, [V, U32, I, U64, V, V, V]),
        "vsa_result_partition_device": (I, [V, U32, I, U64, V, V]),
        "vsa_findmaximaluniquematches": (I, [V, U64, PP]),
        "vsa_findmaximaluniquematches_range": (I, [V, U64, U64, U64, PP]),
        "vsa_findmaximalrepeats": (I, [V, U64, PP]),
        "vsa_findmaximalrepeats_cb": (I, [V, U64, PROCESSMATCH, V]),
        "vsa_findsupermaximalrepeats": (I, [V, U64, PP]),
        "vsa_findsupermaximalrepeats_cb": (I, [V, U64, PROCESSMATCH, V]),
        "vsa_findtandems": (I, [V, U64, PP]),
        "vsa_findmumcandidates_packed": (I, [V, V, U64, C.c_uint32, PP]),
        "vsa_findmumcandidates_grouped": (
            I, [V, V, U64, C.c_uint32, U32, I, V, U64, V, PP]),
        "vsa_result_packbits": (C.c_uint32, [V]),
        "vsa_mumuniqueinquery_range_packed": (
            I, [V, U64, C.c_uint32, U64, I, U64, PP]),
        "vsa_mumuniqueinquery_range_packed2": (
            I, [V, U64, V, U64, C.c_uint32, U64, I, U64, PP]),
        "vsa_findtandems_cb": (I, [V, U64, PROCESSMATCH, V]),
        "vsa_findcompletematches_cb": (I, [V, V, PROCESSMATCH, V]),
        "vsa_findquerymatches_cb": (I, [V, V, I, I, U64, PROCESSMATCH, V]),
        "vsa_findmaximaluniquematches_cb": (I, [V, U64, PROCESSMATCH, V]),
        "vsa_measure_random_read": (I, [U64, I, I, C.POINTER(C.c_double)]),
        "vsa_measure_table_read": (I, [V, I, I, C.POINTER(C.c_double)]),
        "vsa_sink_open": (I, [C.POINTER(SinkParams), PP]),
        "vsa_sink_close": (None, [V]),
        "vsa_sink_format": (C.c_int64, [V, V, U64, V, U64]),
        "vsa_sink_write": (I, [V, V, U64, V]),
        "vsa_splitmix64_at": (U64, [U64, U64]),
        "vsa_synth_genome": (None, [U64, U64, V]),
        "vsa_synth_query_plan": (None, [U64, U64, U64, U32, V, V, V]),
        "vsa_synth_queries": (None, [U64, V, U64, U64, U32, V, V]),
        "vsa_synth_genome_device": (I, [U64, U64, V, I]),
        "vsa_synth_queries_device": (I, [V, U64, V, V, V, U64, U32, V, I]),
        "vsa_device_malloc": (I, [U64, I, PP]),
        "vsa_device_free": (I, [V, I]),
        "vsa_device_upload": (I, [V, V, U64, I]),
        "vsa_device_download": (I, [V, V, U64, I]),
        "vsa_device_count": (I, []),
        "vsa_device_synchronize": (I, [I]),
        "vsa_device_trim": (I, [I]),
        "vsa_device_meminfo": (I, [I, C.POINTER(U64), C.POINTER(U64)]),
        "vsa_measure_stream_read": (I, [U64, I, C.POINTER(C.c_double)]),
        "vsa_coverage_open_index": (I, [V, PP]),
        "vsa_coverage_open_queries": (I, [V, PP]),
        "vsa_coverage_close": (None, [V]),
        "vsa_coverage_numofbits": (U64, [V]),
        "vsa_coverage_coop_threshold": (U64, []),
        "vsa_coverage_mark": (I, [V, V, C.POINTER(CoverageParams)]),
        "vsa_coverage_merge": (I, [V, V]),
        "vsa_coverage_getstats": (I, [V, C.POINTER(CoverageStats)]),
        "vsa_coverage_fetch_bits": (I, [V, V, U64]),
        "vsa_coverage_device_bits": (V, [V]),
        "vsa_coverage_nomatch": (I, [V, U64, U64, U64, PP]),
        "vsa_coverage_nomatch_all": (I, [V, U64, PP]),
        "vsa_coverage_nomatch_database": (I, [V, U64, PP]),
        "vsa_coverage_nomatch_queries": (I, [V, U64, PP]),
        "vsa_nomatch_format": (C.c_int64, [V, U64, U32, U64, V, U64]),
        "vsa_mask_apply": (I, [V, U64, V, I, C.POINTER(U64)]),
        "vsa_select_open": (I, [C.POINTER(SinkParams), V,
                                C.POINTER(SelectParams), I, PP]),
        "vsa_select_add": (I, [V, V, I]),
        "vsa_select_finish": (I, [V, PP]),
        "vsa_select_flags": (I, [V, V, U64]),
        "vsa_select_getstats": (I, [V, C.POINTER(SelectStats)]),
        "vsa_select_evalues": (I, [V, V, I, V, U64]),
        "vsa_select_passes": (U64, [V]),
        "vsa_select_close": (None, [V]),
        "vsa_select_host": (I, [C.POINTER(SinkParams),
                                C.POINTER(SelectParams), V, V, U64, V, V, V,
                                U64, C.POINTER(U64),
                                C.POINTER(SelectStats)]),
        "vsa_cluster_open": (I, [C.POINTER(SinkParams),
                                 C.POINTER(ClusterParams), I, PP]),
        "vsa_cluster_add": (I, [V, V, I]),
        "vsa_cluster_finish": (I, [V]),
        "vsa_cluster_getstats": (I, [V, C.POINTER(ClusterStats)]),
        "vsa_cluster_members": (I, [V, V, V]),
        "vsa_cluster_labels": (I, [V, V]),
        "vsa_cluster_edges": (I, [V, PP, V, V]),
        "vsa_cluster_format": (C.c_int64, [V, V, U64]),
        "vsa_cluster_times": (I, [V, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)]),
        "vsa_cluster_close": (None, [V]),
        "vsa_cluster_host": (I, [C.POINTER(SinkParams),
                                 C.POINTER(ClusterParams), V, V, U64,
                                 C.POINTER(ClusterStats), V, V, V, V, V, V,
                                 U64, C.POINTER(C.c_int64)]),
        "vsa_matchcluster_open": (I, [C.POINTER(SinkParams),
                                      C.POINTER(MatchClusterParams), I, PP]),
        "vsa_matchcluster_add": (I, [V, V, I]),
        "vsa_matchcluster_finish": (I, [V]),
        "vsa_matchcluster_getstats": (I, [V, C.POINTER(MatchClusterStats)]),
        "vsa_matchcluster_members": (I, [V, V, V]),
        "vsa_matchcluster_labels": (I, [V, V]),
        "vsa_matchcluster_edges": (I, [V, V, V, V, V]),
        "vsa_matchcluster_records": (I, [V, PP, V]),
        "vsa_matchcluster_format": (C.c_int64, [V, V, U64]),
        "vsa_matchcluster_format_cluster": (C.c_int64, [V, V, U64, V, U64]),
        "vsa_matchcluster_times": (I, [V, V]),
        "vsa_matchcluster_close": (None, [V]),
        "vsa_matchcluster_host": (I, [C.POINTER(SinkParams),
                                      C.POINTER(MatchClusterParams), V, V,
                                      U64, C.POINTER(MatchClusterStats), V, V,
                                      V, V, V, V, V, U64, V, U64,
                                      C.POINTER(C.c_int64)]),
        "vsa_matchcluster_format_host": (C.c_int64, [V, I, V, V, U64, V, V,
                                                     V, U64, V, U64]),
        "vsa_eratecluster_open": (I, [C.POINTER(SinkParams), V, C.c_uint32,
                                      I, PP]),
        "vsa_eratecluster_host": (I, [C.POINTER(SinkParams), C.c_uint32, V,
                                      U64, V, U64,
                                      C.POINTER(MatchClusterStats), V, V, V,
                                      V, V, V, V, U64, V, U64,
                                      C.POINTER(C.c_int64)]),
        "vsa_sink_setdigits": (I, [V, I, I, I, I, I]),
        "vsa_chain_open": (I, [C.POINTER(SinkParams), C.POINTER(ChainParams),
                               I, PP]),
        "vsa_chain_add": (I, [V, V, I]),
        "vsa_chain_finish": (I, [V]),
        "vsa_chain_getstats": (I, [V, C.POINTER(ChainStats)]),
        "vsa_chain_chains": (I, [V, V, V, V, V]),
        "vsa_chain_members": (I, [V, V]),
        "vsa_chain_records": (I, [V, PP, V]),
        "vsa_chain_format": (C.c_int64, [V, V, I, V, U64]),
        "vsa_chain_times": (I, [V, V]),
        "vsa_chain_close": (None, [V]),
        "vsa_chain_host": (I, [C.POINTER(SinkParams), C.POINTER(ChainParams),
                               V, V, U64, C.POINTER(ChainStats), V, V, V, V,
                               U64, V, U64]),
        "vsa_chain_format_host": (C.c_int64, [V, I, U64, V, V, V, V, V,
                                              U64]),
        "vsa_transnum_check": (I, [U32]),
        "vsa_translate_host": (I, [U32, V, U64, V, V, U64, V, V, U64, V, V,
                                   C.POINTER(U64)]),
        "vsa_queries_translate": (I, [U32, V, U64, V, V, U64, V, I, PP]),
        "vsa_queries_translate_device": (I, [U32, V, U64, U32, V, I, PP]),
        "vsa_queries_download": (I, [V, V, V, V]),
        "vsa_translate_tile": (U64, []),
        "vsa_queries_translate_ms": (C.c_double, [V]),
        "vsa_translated_convert": (I, [V, V, PP, V, U64]),
        "vsa_translated_convert_host": (I, [V, U64, V, U64, U64, V, V]),
        "vsa_extend_maxdist": (U32, []),
        "vsa_extend_lane_budget": (U32, []),
        "vsa_extend_long_step": (U32, []),
        "vsa_extend_seedlength": (U64, [U64, U64, U64]),
        "vsa_extend_hamming": (I, [V, V, V, C.POINTER(SinkParams), I, U64,
                                   U64, U64, PP]),
        "vsa_findquerymatches_hamming": (I, [V, V, U64, U64, U64, I, PP]),
        "vsa_findselfmatches_hamming": (I, [V, U64, U64, U64, PP]),
        "vsa_extend_hamming_host": (I, [C.POINTER(SinkParams), V, V, V, U64,
                                        U64, U64, U64, I, V, U64,
                                        C.POINTER(U64)]),
    }
    # the entries of include/vstree_amd_edist.h
    edist = {
        "vsa_extend_edist_maxdist": (U32, []),
        "vsa_extend_edist": sig["vsa_extend_hamming"],
        "vsa_findquerymatches_edist": sig["vsa_findquerymatches_hamming"],
        "vsa_findselfmatches_edist": sig["vsa_findselfmatches_hamming"],
        "vsa_extend_edist_host": sig["vsa_extend_hamming_host"],
    }
    # the entries of include/vstree_amd_xdrop.h: the flag `hamming` follows
    # the bound X
    xdrop = {
        "vsa_extend_xdrop_seedlength": (U64, [U64]),
        "vsa_extend_xdrop": (I, [V, V, V, C.POINTER(SinkParams), I, U64, U64,
                                 I, U64, PP]),
        "vsa_findquerymatches_xdrop": (I, [V, V, U64, U64, I, U64, I, PP]),
        "vsa_findselfmatches_xdrop": (I, [V, U64, U64, I, U64, PP]),
        "vsa_extend_xdrop_host": (I, [C.POINTER(SinkParams), V, V, V, U64,
                                      U64, U64, I, U64, I, V, U64,
                                      C.POINTER(U64)]),
    }
    # the entries of include/vstree_amd_align.h
    align = {
        "vsa_align_maxdist": (U32, []),
        "vsa_align": (I, [V, V, V, C.POINTER(SinkParams), I, PP]),
        "vsa_alignments_info": (I, [V, C.POINTER(AlignStats)]),
        "vsa_alignments_fetch": (I, [V, V, V]),
        "vsa_alignments_free": (None, [V]),
        "vsa_align_host": (I, [C.POINTER(SinkParams), V, V, V, U64, I, I, V,
                               V, U64]),
        "vsa_align_format": (C.c_int64, [V, V, U64, V, V, V, V, V, V, U32, V,
                                         U64]),
        "vsa_align_write": (I, [V, V, U64, V, V, V, V, V, V, U32, V]),
    }
    # the entries of include/vstree_amd_online.h
    online = {
        "vsa_text_from_host": (I, [V, U64, U32, I, PP]),
        "vsa_text_from_device": (I, [V, U64, U32, I, PP]),
        "vsa_text_open": (I, [C.c_char_p, I, PP]),
        "vsa_text_close": (None, [V]),
        "vsa_findcompletematches_online": (I, [V, V, I, U64, I, I, PP]),
        "vsa_text_findcompletematches_online": (I, [V, V, I, U64, I, I, PP]),
        "vsa_findcompletematches_online_host": (
            I, [V, U64, V, V, V, U64, U64, I, U64, I, I, I, V, U64,
                C.POINTER(U64)]),
        "vsa_online_plan": (I, [U64, U64, I, C.POINTER(U32), C.POINTER(U64),
                                C.POINTER(U64), C.POINTER(U64)]),
    }
    for name, (res, args) in list(sig.items()) + list(edist.items()) + \
            list(xdrop.items()) + list(align.items()) + list(online.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return (lib, sorted(sig), sorted(edist), sorted(xdrop), sorted(align),
            sorted(online))


(lib, ABI_SYMBOLS, EDIST_ABI_SYMBOLS, XDROP_ABI_SYMBOLS,
 ALIGN_ABI_SYMBOLS, ONLINE_ABI_SYMBOLS) = _load()


def messagespace():
    return lib.vsa_messagespace().decode(errors="replace")


def _check(rc):
    if rc != 0:
        raise VsaError(rc, messagespace())


def _ptr(a):
    return None if a is None else a.ctypes.data


class Index:
    """An enhanced suffix array resident in one GPU's HBM (vsa_index)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_tables(cls, totallength, prefixlength, numofchars, tis, suf, lcp,
                    llv, bck, bwt=None, querysepposition=0,
                    hasindexedqueries=False, device=0):
        suf = np.ascontiguousarray(suf)
        assert suf.dtype in (np.uint32, np.uint64)
        tis = np.ascontiguousarray(tis, np.uint8)
        lcp = np.ascontiguousarray(lcp, np.uint8)
        llv = np.ascontiguousarray(llv, suf.dtype)
        bck = np.ascontiguousarray(bck, suf.dtype)
        bwt = None if bwt is None else np.ascontiguousarray(bwt, np.uint8)
        t = Tables(int(totallength), int(prefixlength), int(numofchars),
                   suf.dtype.itemsize * 8, llv.shape[0] // 2, _ptr(tis),
                   _ptr(suf), _ptr(lcp), _ptr(llv), _ptr(bck), _ptr(bwt),
                   int(querysepposition), int(bool(hasindexedqueries)))
        h = C.c_void_p()
        _check(lib.vsa_index_from_tables(C.byref(t), device, C.byref(h)))
        return cls(h)

    @classmethod
    def open(cls, indexname, device=0):
        """mapvirtualtreeifyoucan + upload (vsa_index_open)."""
        h = C.c_void_p()
        _check(lib.vsa_index_open(os.fsencode(indexname), device,
                                  C.byref(h)))
        return cls(h)

    @classmethod
    def build(cls, tis, numofchars=4, prefixlength=0, device=0):
        tis = np.ascontiguousarray(tis, np.uint8)
        h = C.c_void_p()
        _check(lib.vsa_index_build(_ptr(tis), tis.shape[0], numofchars,
                                   prefixlength, device, C.byref(h)))
        return cls(h)

    @classmethod
    def build_device(cls, device_tis, totallength, numofchars=4,
                     prefixlength=0, device=0):
        h = C.c_void_p()
        _check(lib.vsa_index_build_device(device_tis, totallength, numofchars,
                                          prefixlength, device, C.byref(h)))
        return cls(h)

    def info(self):
        i = IndexInfo()
        _check(lib.vsa_index_getinfo(self._h, C.byref(i)))
        return i

    def download(self, with_bwt=True):
        """-> dict of numpy arrays with the device tables."""
        i = self.info()
        dt = np.uint32 if i.device_integersize == 32 else np.uint64
        n = i.totallength
        out = {"tis": np.zeros(n, np.uint8), "suf": np.zeros(n + 1, dt),
               "lcp": np.zeros(n + 1, np.uint8),
               "llv": np.zeros(2 * i.largelcpvalues, dt),
               "bck": np.zeros(2 * i.numofcodes, dt),
               "bwt": (np.zeros(n + 1, np.uint8)
                       if (with_bwt and i.hasbwt) else None)}
        _check(lib.vsa_index_download(self._h, _ptr(out["tis"]),
                                      _ptr(out["suf"]), _ptr(out["lcp"]),
                                      _ptr(out["llv"]), _ptr(out["bck"]),
                                      _ptr(out["bwt"])))
        return out

    def clone(self, device=0):
        """replica on another device: device-to-device copies, no rebuild"""
        h = C.c_void_p()
        _check(lib.vsa_index_clone(self._h, int(device), C.byref(h)))
        return Index(h)

    def set_queryseparator(self, pos):
        _check(lib.vsa_index_set_queryseparator(self._h, int(pos)))

    def set_queryspeedup(self, level):
        """vmatch -qspeedup: 0 or 2 (default), the order of MEM lists."""
        _check(lib.vsa_index_set_queryspeedup(self._h, int(level)))

    def make_sti1(self):
        out = np.zeros(self.info().totallength + 1, np.uint8)
        _check(lib.vsa_index_make_sti1(self._h, _ptr(out)))
        return out

    def close(self):
        if self._h and lib is not None:   # None at interpreter shutdown
            lib.vsa_index_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Queries:
    """A batch of query sequences resident in HBM (vsa_queries)."""

    def __init__(self, handle, nq):
        self._h = handle
        self.nq = nq

    @classmethod
    def from_host(cls, symbols, start, length, device=0):
        symbols = np.ascontiguousarray(symbols, np.uint8)
        start = np.ascontiguousarray(start, np.uint64)
        length = np.ascontiguousarray(length, np.uint64)
        h = C.c_void_p()
        _check(lib.vsa_queries_from_host(_ptr(symbols), symbols.shape[0],
                                         _ptr(start), _ptr(length),
                                         start.shape[0], device, C.byref(h)))
        return cls(h, start.shape[0])

    @classmethod
    def from_host_packed(cls, symbols, m, device=0, stride=None):
        """nq reads of m mapped symbols (read i at symbols[i * stride:]) ->
        packed on the host (vsa_pack_reads), uploaded as rows + side list"""
        symbols = np.ascontiguousarray(symbols, np.uint8)
        stride = m if stride is None else stride
        nq = 0 if len(symbols) < m else (len(symbols) - m) // stride + 1
        rows, special, ns = pack_reads(symbols, nq, m, stride)
        h = C.c_void_p()
        _check(lib.vsa_queries_from_host_packed(
            _ptr(rows), nq, m, _ptr(special), ns, device, C.byref(h)))
        return cls(h, nq)

    @classmethod
    def from_device(cls, device_symbols, nq, m, device=0):
        h = C.c_void_p()
        _check(lib.vsa_queries_from_device(device_symbols, nq, m, device,
                                           C.byref(h)))
        return cls(h, nq)

    @classmethod
    def translate(cls, transnum, dnachars, start, length, symbolmap,
                  device=0):
        """vmatch -dnavsprot transnum: the six reading frames of DNA sequences
        given as CHARACTERS (sequence i = dnachars[start[i]:start[i] +
        length[i]]) as a batch of 6 * len(start) protein queries under the
        symbol map of the index (vsa_queries_translate)"""
        dnachars = np.ascontiguousarray(dnachars, np.uint8)
        start = np.ascontiguousarray(start, np.uint64)
        length = np.ascontiguousarray(length, np.uint64)
        symbolmap = np.ascontiguousarray(symbolmap, np.uint8)
        assert symbolmap.shape == (256,)
        h = C.c_void_p()
        _check(lib.vsa_queries_translate(
            int(transnum), _ptr(dnachars), dnachars.shape[0], _ptr(start),
            _ptr(length), start.shape[0], _ptr(symbolmap), device,
            C.byref(h)))
        return cls(h, 6 * start.shape[0])

    @classmethod
    def translate_device(cls, transnum, device_chars, nq, m, symbolmap,
                         device=0):
        """the same for nq reads of m characters back to back in device
        memory (vsa_queries_translate_device)"""
        symbolmap = np.ascontiguousarray(symbolmap, np.uint8)
        assert symbolmap.shape == (256,)
        h = C.c_void_p()
        _check(lib.vsa_queries_translate_device(
            int(transnum), device_chars, int(nq), int(m), _ptr(symbolmap),
            device, C.byref(h)))
        return cls(h, 6 * int(nq))

    def translate_ms(self):
        """HIP-event time of the translation kernels of a translated batch"""
        return float(lib.vsa_queries_translate_ms(self._h))

    def download(self):
        """-> (symbols, start, length) of a byte batch as numpy arrays"""
        qi = self.info()
        sym = np.zeros(qi.numofsymbols, np.uint8)
        start = np.zeros(qi.numofqueries, np.uint64)
        length = np.zeros(qi.numofqueries, np.uint64)
        _check(lib.vsa_queries_download(self._h, _ptr(sym), _ptr(start),
                                        _ptr(length)))
        return sym, start, length

    def set_offset(self, offset):
        """(a translated batch counts six-frame sequences: 6 * first read)"""
        _check(lib.vsa_queries_set_offset(self._h, int(offset)))

    def info(self):
        qi = QueriesInfo()
        _check(lib.vsa_queries_getinfo(self._h, C.byref(qi)))
        return qi

    def reverse_complement(self):
        """vmatch -p: every sequence reversed and complemented on its own"""
        h = C.c_void_p()
        _check(lib.vsa_queries_reverse_complement(self._h, C.byref(h)))
        return Queries(h, self.nq)

    def close(self):
        if self._h and lib is not None:
            lib.vsa_queries_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


class Result:
    """A match list resident in HBM (vsa_result)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, matches, device=0):
        """a MATCH_DTYPE array as a match list on the device"""
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        h = C.c_void_p()
        _check(lib.vsa_result_from_host(_ptr(matches), len(matches), device,
                                        C.byref(h)))
        return cls(h)

    @property
    def count(self):
        return int(lib.vsa_result_count(self._h))

    def stats(self):
        s = Stats()
        _check(lib.vsa_result_getstats(self._h, C.byref(s)))
        return s

    def copy_device(self, device_ptr, capacity):
        _check(lib.vsa_result_copy_device(self._h, device_ptr, capacity))

    def partition(self, nparts, totallength, device_ptr, own=-1):
        """records grouped by the index range of their dbstart, written to
        device_ptr; -> (number of records, largest right end) per part.
        own >= 0: that part lies behind all others"""
        counts = np.zeros(nparts, np.uint64)
        maxright = np.zeros(nparts, np.uint64)
        _check(lib.vsa_result_partition_own(self._h, int(nparts), int(own),
                                            int(totallength), device_ptr,
                                            _ptr(counts), _ptr(maxright)))
        return counts, maxright

    def partition_device(self, nparts, totallength, device_ptr, device_meta,
                         own=-1):
        """partition() that leaves (counts, largest right ends) in device
        memory at device_meta (2*nparts uint64) and does not wait for the
        GPU"""
        _check(lib.vsa_result_partition_device(
            self._h, int(nparts), int(own), int(totallength), device_ptr,
            device_meta))

    @property
    def packbits(self):
        """length bits of a packed candidate result, 0 for records"""
        return int(lib.vsa_result_packbits(self._h))

    @property
    def rowwords(self):
        """8-byte words per row that partition() writes"""
        return 2 if self.packbits else 4

    def fetch(self):
        n = self.count
        out = np.zeros(n, MATCH_DTYPE)
        if n:
            _check(lib.vsa_result_fetch(self._h, _ptr(out), n))
        return out

    def close(self):
        if self._h and lib is not None:
            lib.vsa_result_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def findcompletematches(index, queries):
    """vmatch -complete -q (Vmengine/fcomplete.c:263).  On the reference's
    short-query error the VsaError carries the matches found before it in
    .partial."""
    h = C.c_void_p()
    rc = lib.vsa_findcompletematches(index._h, queries._h, C.byref(h))
    res = Result(h) if h else None
    if rc != 0:
        e = VsaError(rc, messagespace())
        e.partial = res
        raise e
    return res


NOT_COVERED = -4


def findapproxcompletematches(index, queries, doedist, distvalue,
                              percent=False):
    """vmatch -complete -e K | -h K -q (Vmengine/approxcompl.c:138); the
    distance of a match travels in its querystart field.  VsaError.code ==
    NOT_COVERED: a configuration the engine leaves to the CPU reference."""
    h = C.c_void_p()
    rc = lib.vsa_findapproxcompletematches(index._h, queries._h,
                                           int(doedist), int(distvalue),
                                           int(percent), C.byref(h))
    res = Result(h) if h else None
    if rc != 0:
        e = VsaError(rc, messagespace())
        e.partial = res
        raise e
    return res


def findquerymatches(index, queries, searchlength, mum=False, cand=False,
                     speedup=None):
    """vmatch [-mum [cand]] -l L -q (Vmengine/fquery.c:1009); speedup = the
    -qspeedup level (0 or 2) to set on the index first."""
    if speedup is not None:
        index.set_queryspeedup(speedup)
    h = C.c_void_p()
    _check(lib.vsa_findquerymatches(index._h, queries._h, int(mum),
                                    int(cand), int(searchlength),
                                    C.byref(h)))
    return Result(h)


def findmumcandidates(index, queries, searchlength, ordered=True):
    """vmatch -mum cand; ordered=False: as the kernel left them (for a
    filter that sorts them anyway)"""
    h = C.c_void_p()
    _check(lib.vsa_findmumcandidates(index._h, queries._h, int(searchlength),
                                     int(ordered), C.byref(h)))
    return Result(h)


def findmumcandidates_packed(index, queries, searchlength, lengthbits=0):
    """the candidates as (sort key, value) pairs for the multi-GPU filter,
    see the header"""
    h = C.c_void_p()
    _check(lib.vsa_findmumcandidates_packed(index._h, queries._h,
                                            int(searchlength),
                                            int(lengthbits), C.byref(h)))
    return Result(h)


def findmumcandidates_grouped(index, queries, searchlength, lengthbits,
                              nparts, own, device_rows, capacity,
                              device_meta):
    """findmumcandidates_packed + Result.partition_device in one call ->
    (result, grouped): grouped False = more than `capacity` rows, nothing
    was written to device_rows"""
    h = C.c_void_p()
    rc = lib.vsa_findmumcandidates_grouped(
        index._h, queries._h, int(searchlength), int(lengthbits),
        int(nparts), int(own), device_rows, int(capacity), device_meta,
        C.byref(h))
    if rc not in (0, 1):
        _check(rc)
    return Result(h), rc == 0


def findmaximalrepeats(index, searchlength):
    """vmatch -l L IDX (Vmengine/vmatfind.c:487), the reference's order."""
    h = C.c_void_p()
    _check(lib.vsa_findmaximalrepeats(index._h, int(searchlength),
                                      C.byref(h)))
    return Result(h)


def findsupermaximalrepeats(index, searchlength):
    """vmatch -supermax -l L IDX (Vmengine/fsuper.c:142)."""
    h = C.c_void_p()
    _check(lib.vsa_findsupermaximalrepeats(index._h, int(searchlength),
                                           C.byref(h)))
    return Result(h)


def findtandems(index, searchlength):
    """vmatch -tandem -l L IDX (Vmengine/ftandem.c:261)."""
    h = C.c_void_p()
    _check(lib.vsa_findtandems(index._h, int(searchlength), C.byref(h)))
    return Result(h)


def findmaximaluniquematches(index, searchlength, first=None, last=None):
    """vmatch -mum -l L IDX (Vmengine/fmumself.c:10); first/last: the part
    first <= i < last of the reference's scan (multi-GPU form)."""
    h = C.c_void_p()
    if first is None and last is None:
        _check(lib.vsa_findmaximaluniquematches(index._h, int(searchlength),
                                                C.byref(h)))
    else:
        _check(lib.vsa_findmaximaluniquematches_range(
            index._h, int(searchlength), int(first or 0),
            int(last if last is not None else 2 ** 64 - 1), C.byref(h)))
    return Result(h)


def mumuniqueinquery(device_candidates, ncandidates, device=0):
    """kurtz/cleanMUMcand.c:55 on candidates resident in device memory."""
    h = C.c_void_p()
    _check(lib.vsa_mumuniqueinquery(device_candidates, int(ncandidates),
                                    device, C.byref(h)))
    return Result(h)


def mumuniqueinquery_range(device_candidates, ncandidates, carry_dbright,
                           device=0):
    """the filter on one dbstart range (multi-GPU), see the header"""
    h = C.c_void_p()
    _check(lib.vsa_mumuniqueinquery_range(device_candidates,
                                          int(ncandidates), device,
                                          int(carry_dbright), C.byref(h)))
    return Result(h)


def mumuniqueinquery_range_packed(device_rows, nrows, lengthbits, totallength,
                                  carry_dbright, device=0):
    """the filter on one dbstart range of packed candidate rows"""
    h = C.c_void_p()
    _check(lib.vsa_mumuniqueinquery_range_packed(
        device_rows, int(nrows), int(lengthbits), int(totallength), device,
        int(carry_dbright), C.byref(h)))
    return Result(h)


def mumuniqueinquery_range_packed2(device_rows, nrows, more_rows, nmore,
                                   lengthbits, totallength, carry_dbright,
                                   device=0):
    """the filter on one dbstart range of packed candidate rows that lie in
    two places (own rows, received rows)"""
    h = C.c_void_p()
    _check(lib.vsa_mumuniqueinquery_range_packed2(
        device_rows, int(nrows), more_rows, int(nmore), int(lengthbits),
        int(totallength), device, int(carry_dbright), C.byref(h)))
    return Result(h)


def _collector(stop_after=None):
    got = []

    def cb(info, mptr):
        m = np.frombuffer((C.c_uint64 * 4).from_address(mptr), np.uint64)
        got.append(tuple(int(x) for x in m))
        if stop_after is not None and len(got) >= stop_after:
            return 1
        return 0
    return got, PROCESSMATCH(cb)


def findcompletematches_cb(index, queries, stop_after=None):
    got, cb = _collector(stop_after)
    rc = lib.vsa_findcompletematches_cb(index._h, queries._h, cb, None)
    return rc, got


def findapproxcompletematches_cb(index, queries, doedist, distvalue,
                                 percent=False, stop_after=None):
    got, cb = _collector(stop_after)
    rc = lib.vsa_findapproxcompletematches_cb(
        index._h, queries._h, int(doedist), int(distvalue), int(percent), cb,
        None)
    return rc, got


def findquerymatches_cb(index, queries, searchlength, mum=False, cand=False,
                        stop_after=None, speedup=None):
    if speedup is not None:
        index.set_queryspeedup(speedup)
    got, cb = _collector(stop_after)
    rc = lib.vsa_findquerymatches_cb(index._h, queries._h, int(mum),
                                     int(cand), int(searchlength), cb, None)
    return rc, got


def findmaximaluniquematches_cb(index, searchlength, stop_after=None):
    got, cb = _collector(stop_after)
    rc = lib.vsa_findmaximaluniquematches_cb(index._h, int(searchlength), cb,
                                             None)
    return rc, got


class Pipeline:
    """vsa_pipeline_*: host memory in, host memory out, three batches in
    flight.  mode: 0 -complete, 1 MEM, 2 -mum cand, 3 -mum."""

    def __init__(self, index, mode, searchlength, querylength, maxqueries,
                 packed=False, maxspecial=None):
        self._h = None
        h = C.c_void_p()
        self.packed = bool(packed)
        self.maxspecial = int(maxqueries if maxspecial is None
                              else maxspecial)
        if packed:
            _check(lib.vsa_pipeline_open_packed(
                index._h, int(mode), int(searchlength), int(querylength),
                int(maxqueries), self.maxspecial, C.byref(h)))
        else:
            _check(lib.vsa_pipeline_open(index._h, int(mode),
                                         int(searchlength), int(querylength),
                                         int(maxqueries), C.byref(h)))
        self._h, self._index = h, index
        self.m, self.maxqueries = int(querylength), int(maxqueries)
        self.W = int(lib.vsa_packed_words(self.m))

    def hostrows(self):
        """packed pipelines: (rows, special) numpy views of the page-locked
        room of the next batch, or None when all batches are in flight"""
        r, sp = C.c_void_p(), C.c_void_p()
        rc = lib.vsa_pipeline_hostrows(self._h, C.byref(r), C.byref(sp))
        if rc == 1:
            return None
        _check(rc)
        rows = np.ctypeslib.as_array(
            (C.c_uint64 * (self.W * self.maxqueries)).from_address(r.value))
        special = np.ctypeslib.as_array(
            (C.c_uint8 * max(1, self.m * self.maxspecial)).from_address(
                sp.value))
        return rows, special

    def pack_into_slot(self, symbols, nq, stride=None):
        """packs nq reads into the next slot and submits it; False when all
        batches are in flight"""
        got = self.hostrows()
        if got is None:
            return False
        rows, special = got
        ns = C.c_uint64(0)
        symbols = np.ascontiguousarray(symbols, np.uint8)
        _check(lib.vsa_pack_reads(_ptr(symbols), nq, self.m,
                                  self.m if stride is None else stride,
                                  _ptr(rows), _ptr(special), self.maxspecial,
                                  C.byref(ns)))
        _check(lib.vsa_pipeline_submit_packed(self._h, int(nq),
                                              int(ns.value)))
        return True

    def hostbuffer(self):
        """numpy view of the page-locked buffer of the next batch, or None
        when all batches are in flight"""
        p = lib.vsa_pipeline_hostbuffer(self._h)
        if not p:
            return None
        return np.ctypeslib.as_array(
            (C.c_uint8 * (self.m * self.maxqueries)).from_address(p))

    def submit(self, nq):
        _check(lib.vsa_pipeline_submit(self._h, int(nq)))

    def next(self, copy=True):
        """-> (rc, matches): rc 1 = nothing outstanding"""
        ptr, n = C.c_void_p(), C.c_uint64()
        rc = lib.vsa_pipeline_next(self._h, C.byref(ptr), C.byref(n))
        if rc == 1 or n.value == 0:
            return rc, np.zeros(0, MATCH_DTYPE)
        a = np.ctypeslib.as_array(
            (C.c_uint64 * (4 * n.value)).from_address(ptr.value)).view(
                MATCH_DTYPE)
        return rc, a.copy() if copy else a

    def finish(self, copy=True, compact=False):
        """compact: vsa_pipeline_finish16 -> an array of MATCH16_DTYPE
        (expand_match16 gives the records)"""
        ptr, n, st = C.c_void_p(), C.c_uint64(), Stats()
        if compact:
            _check(lib.vsa_pipeline_finish16(self._h, C.byref(ptr),
                                             C.byref(n), C.byref(st)))
            if n.value == 0:
                return np.zeros(0, MATCH16_DTYPE), st
            a = np.ctypeslib.as_array(
                (C.c_uint64 * (2 * n.value)).from_address(ptr.value)).view(
                    MATCH16_DTYPE)
            return (a.copy() if copy else a), st
        _check(lib.vsa_pipeline_finish(self._h, C.byref(ptr), C.byref(n),
                                       C.byref(st)))
        if n.value == 0:
            return np.zeros(0, MATCH_DTYPE), st
        a = np.ctypeslib.as_array(
            (C.c_uint64 * (4 * n.value)).from_address(ptr.value)).view(
                MATCH_DTYPE)
        return (a.copy() if copy else a), st

    def close(self):
        if self._h and lib is not None:
            lib.vsa_pipeline_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- host match sink ------------------------------------------------------

SINK_COMPLETE, SINK_QUERY, SINK_SELF, SINK_APPROX_EDIST, \
    SINK_APPROX_HAMMING = range(5)
# vmatch -dnavsprot: records of a six-frame batch (Queries.translate), the
# query Multiseq of the layout is the DNA one; lines with the flags F / G
# (_COMPLETE: the records of findcompletematches on such a batch)
SINK_TRANSLATED, SINK_TRANSLATED_COMPLETE = 5, 6
# vmatch -l L -h K outside -complete: records of extended seeds, the distance
# in the top 16 bits of the length (hamming_lengths / hamming_distances)
SINK_QUERY_HAMMING, SINK_SELF_HAMMING = 8, 9
SHOW_ABSOLUTE, SHOW_NODIST, SHOW_NOEVALUE, SHOW_NOSCORE, SHOW_NOIDENTITY = (
    1, 2, 4, 8, 16)


def sink_params(kind, totallength, markpos, numofchars=4, querystart=None,
                querylength=None, querytotallength=0, numofquerysequences=0,
                totalquerylength=0, leastlength=0, palindromic=False,
                showmode=0, threads=0, selfpalindromic=False):
    """the description of a run (vsa_sinkparams) for Sink and Select ->
    (SinkParams, the arrays it points into)"""
    keep = [np.ascontiguousarray(markpos, np.uint64)]
    p = SinkParams()
    p.kind, p.palindromic = int(kind), int(bool(palindromic))
    p.selfpalindromic = int(bool(selfpalindromic))
    p.showmode, p.numofchars = int(showmode), int(numofchars)
    p.threads = int(threads)
    p.leastlength, p.totallength = int(leastlength), int(totallength)
    p.numofsequences = keep[0].shape[0] + 1
    p.markpos = _ptr(keep[0]) if keep[0].shape[0] else None
    p.numofquerysequences = int(numofquerysequences)
    p.totalquerylength = int(totalquerylength)
    if querystart is not None:
        qs = np.ascontiguousarray(querystart, np.uint64)
        ql = np.ascontiguousarray(querylength, np.uint64)
        keep += [qs, ql]
        p.numofqueries = qs.shape[0]
        p.querytotallength = int(querytotallength)
        p.querystart, p.querylength = _ptr(qs), _ptr(ql)
    return p, keep


class Sink:
    """vmatch's output lines for match records (vsa_sink, host side)."""

    def __init__(self, *args, **kw):
        p, self._keep = sink_params(*args, **kw)
        self._h = C.c_void_p()
        _check(lib.vsa_sink_open(C.byref(p), C.byref(self._h)))

    def format(self, matches):
        """matches: MATCH_DTYPE array -> bytes (one line per match)"""
        matches = np.ascontiguousarray(matches, MATCH_DTYPE)
        cap = 192 * (matches.shape[0] + 1)
        buf = np.empty(cap, np.uint8)
        n = lib.vsa_sink_format(self._h, _ptr(matches), matches.shape[0],
                                _ptr(buf), cap)
        if n < 0:
            raise VsaError(int(n), messagespace())
        return buf[:n].tobytes()

    def setdigits(self, length=5, position1=6, position2=6, seqnum1=3,
                  seqnum2=3):
        """the field widths of the lines; the defaults are those the
        reference's post-processing prints with (ASSIGNDEFAULTDIGITS)"""
        _check(lib.vsa_sink_setdigits(self._h, length, position1, position2,
                                      seqnum1, seqnum2))

    def close(self):
        if self._h and lib is not None:
            lib.vsa_sink_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


# ---- six-frame translation (vmatch -dnavsprot) ------------------------------

TRANSLATE_TILE = int(lib.vsa_translate_tile())
TRANSLATION_TABLES = (1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22,
                      23)


def transnum_check(transnum):
    """raises the reference's error for an illegal translation table number"""
    _check(lib.vsa_transnum_check(int(transnum)))


def translate_host(transnum, dnachars, start, length, symbolmap):
    """the six-frame translation on the host (vsa_translate_host, no GPU)
    -> (symbols, start, length) of the 6 * len(start) protein sequences"""
    dnachars = np.ascontiguousarray(dnachars, np.uint8)
    start = np.ascontiguousarray(start, np.uint64)
    length = np.ascontiguousarray(length, np.uint64)
    symbolmap = np.ascontiguousarray(symbolmap, np.uint8)
    assert symbolmap.shape == (256,)
    nq = start.shape[0]
    cap = int((length // np.uint64(3)).sum()) * 6 + 6 * nq + 1
    protein = np.zeros(cap, np.uint8)
    pstart, plength = np.zeros(6 * nq, np.uint64), np.zeros(6 * nq, np.uint64)
    n = C.c_uint64(0)
    _check(lib.vsa_translate_host(
        int(transnum), _ptr(dnachars), dnachars.shape[0], _ptr(start),
        _ptr(length), nq, _ptr(symbolmap), _ptr(protein), cap, _ptr(pstart),
        _ptr(plength), C.byref(n)))
    return protein[:n.value].copy(), pstart, plength


def translated_convert(result, protein):
    """a list the engine delivered on a translated batch -> (Result with the
    query view in DNA coordinates, one strand byte per record: 1 = reverse
    frame) (vsa_translated_convert)"""
    n = result.count
    reverse = np.zeros(n, np.uint8)
    h = C.c_void_p()
    _check(lib.vsa_translated_convert(result._h, protein._h, C.byref(h),
                                      _ptr(reverse), n))
    return Result(h), reverse


def translated_convert_host(matches, dnalength, offset=0):
    """the same on a MATCH_DTYPE array in host memory
    (vsa_translated_convert_host) -> (query view, strand bytes)"""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    dnalength = np.ascontiguousarray(dnalength, np.uint64)
    view = np.zeros(matches.shape[0], MATCH_DTYPE)
    reverse = np.zeros(matches.shape[0], np.uint8)
    _check(lib.vsa_translated_convert_host(
        _ptr(matches), matches.shape[0], _ptr(dnalength), dnalength.shape[0],
        int(offset), _ptr(view), _ptr(reverse)))
    return view, reverse


# ---- match coverage (vmatch -dbnomatch / -qnomatch / -dbmaskmatch /
# -qmaskmatch) ---------------------------------------------------------------

COVERAGE_QUERY, COVERAGE_SELF, COVERAGE_APPROX = 0, 1, 2
COVERAGE_DATABASE, COVERAGE_QUERIES = 0, 1
COVERAGE_COOP_THRESHOLD = int(lib.vsa_coverage_coop_threshold())
COVERAGE_EXTRACT_TILE = 65536
MASK_TOUPPER, MASK_TOLOWER = 256, 257
# record of Coverage.nomatch: a run of unmarked positions
INTERVAL_DTYPE = np.dtype([("length", "<u8"), ("start", "<u8"),
                           ("seqnum", "<u8"), ("relstart", "<u8")])
_KEEP = {"keepleft": "markleft", "keepright": "markright",
         "keepleftifsamesequence": "markleftifdifferentsequence",
         "keeprightifsamesequence": "markrightifdifferentsequence"}


def coverage_options(keep=None, withquery=False, option="-dbnomatch"):
    """the four keep flags of `-dbnomatch N [keyword]` / `-dbmaskmatch C
    [keyword]` (Vmatch/keepflags.c:9-27, defaults Vmatch/parsevm.c:83-87) as
    keyword arguments of Coverage.mark; withquery: -q is given, where a
    keyword is the reference's error (parsevm.c:70-80)"""
    flags = {v: 1 for v in _KEEP.values()}
    if keep is not None:
        if keep not in _KEEP:
            raise VsaError(-2, "illegal argument \"%s\" to option %s: "
                           "possible arguments are: keepleft, keepright, "
                           "keepleftifsamesequence, keeprightifsamesequence"
                           % (keep, option))
        if withquery:
            raise VsaError(-2, "argument \"%s\" to option %s not allowed if "
                           "option -q is used" % (keep, option))
        flags[_KEEP[keep]] = 0
    return flags


class Coverage:
    """One bit per position of a Multiseq in HBM (vsa_coverage): the
    reference's marktable.  Coverage.over_index(index) /
    Coverage.over_queries(queries)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def over_index(cls, index):
        h = C.c_void_p()
        _check(lib.vsa_coverage_open_index(index._h, C.byref(h)))
        return cls(h)

    @classmethod
    def over_queries(cls, queries):
        h = C.c_void_p()
        _check(lib.vsa_coverage_open_queries(queries._h, C.byref(h)))
        return cls(h)

    @property
    def nbits(self):
        return int(lib.vsa_coverage_numofbits(self._h))

    def mark(self, result, layout=COVERAGE_QUERY, side=COVERAGE_DATABASE,
             palindromic=False, selfpalindromic=False, complete=False,
             markleft=1, markright=1, markleftifdifferentsequence=1,
             markrightifdifferentsequence=1):
        """markmatches (Vmatch/markmat.c:42) for every record of a Result"""
        p = CoverageParams(int(layout), int(side), int(bool(palindromic)),
                           int(bool(selfpalindromic)), int(bool(complete)),
                           int(markleft), int(markright),
                           int(markleftifdifferentsequence),
                           int(markrightifdifferentsequence))
        _check(lib.vsa_coverage_mark(self._h, result._h, C.byref(p)))

    def merge(self, other):
        _check(lib.vsa_coverage_merge(self._h, other._h))

    def stats(self):
        s = CoverageStats()
        _check(lib.vsa_coverage_getstats(self._h, C.byref(s)))
        return s

    def bits(self):
        """-> the table as uint64 words (position p = bit p & 63 of word
        p >> 6)"""
        out = np.zeros((self.nbits + 63) // 64, np.uint64)
        if len(out):
            _check(lib.vsa_coverage_fetch_bits(self._h, _ptr(out), len(out)))
        return out

    def device_bits(self):
        return lib.vsa_coverage_device_bits(self._h)

    def nomatch(self, minlength, first=None, length=None, part=None):
        """runs of unmarked positions of at least minlength -> array of
        INTERVAL_DTYPE.  part: None (the whole table or [first, first +
        length)), "database" or "queries" of an index with queries"""
        h = C.c_void_p()
        if part == "database":
            rc = lib.vsa_coverage_nomatch_database(self._h, int(minlength),
                                                   C.byref(h))
        elif part == "queries":
            rc = lib.vsa_coverage_nomatch_queries(self._h, int(minlength),
                                                  C.byref(h))
        elif first is None:
            rc = lib.vsa_coverage_nomatch_all(self._h, int(minlength),
                                              C.byref(h))
        else:
            rc = lib.vsa_coverage_nomatch(self._h, int(minlength), int(first),
                                          int(length), C.byref(h))
        _check(rc)
        return Result(h).fetch().view(INTERVAL_DTYPE)

    def close(self):
        if self._h and lib is not None:
            lib.vsa_coverage_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def nomatch_format(intervals, showmode=0, posoffset=0):
    """the reference's lines for runs of unmarked positions (shownomatch,
    Vmatch/nomatch.c:36) -> bytes; posoffset != 0: the query part of an
    index with queries"""
    iv = np.ascontiguousarray(intervals).view(MATCH_DTYPE)
    cap = 64 * (len(iv) + 1)
    buf = np.empty(cap, np.uint8)
    n = lib.vsa_nomatch_format(_ptr(iv), len(iv), int(showmode),
                               int(posoffset), _ptr(buf), cap)
    if n < 0:
        raise VsaError(int(n), messagespace())
    return buf[:n].tobytes()


def mask_apply(bits, chars, maskchar):
    """showmaskedseq (Vmatch/showmasked.c:49) on the characters of a
    Multiseq (separators as SEPARATOR) -> (masked characters, number of
    masked symbols); maskchar: a character, MASK_TOUPPER or MASK_TOLOWER"""
    bits = np.ascontiguousarray(bits, np.uint64)
    out = np.array(np.frombuffer(bytes(chars), np.uint8)
                   if isinstance(chars, (bytes, bytearray))
                   else np.asarray(chars, np.uint8), copy=True)
    assert len(bits) * 64 >= len(out)
    if not isinstance(maskchar, int):
        maskchar = ord(maskchar)
    n = C.c_uint64(0)
    _check(lib.vsa_mask_apply(_ptr(bits), len(out), _ptr(out), maskchar,
                              C.byref(n)))
    return out, int(n.value)


# ---- match selection (vmatch -best, -sort, -evalue, -identity, -leastscore,
# the gap bounds of -l L lo [hi]) ------------------------------------------------

SORT_MODES = ("la", "ld", "ia", "id", "ja", "jd", "ea", "ed", "sa", "sd",
              "ida", "idd")
SORT_NONE = 12
SELECT_TILE = 1024


def select_params(best=0, sort=None, evalue=None, identity=0,
                  leastscore=None, gap=None):
    """-best N, -sort mode (a name of SORT_MODES or its number), -evalue X,
    -identity I, -leastscore S, gap = (lo,) or (lo, hi) -> SelectParams"""
    p = SelectParams()
    p.bestnumber = int(best)
    p.sortmode = SORT_NONE if sort is None else (
        SORT_MODES.index(sort) if isinstance(sort, str) else int(sort))
    if evalue is not None:
        p.hasmaxevalue, p.maximumevalue = 1, float(evalue)
    p.identity = int(identity)
    if leastscore is not None:
        p.hasleastscore, p.leastscore = 1, int(leastscore)
    if gap is not None:
        p.haslowergap, p.lowergap = 1, int(gap[0])
        if len(gap) > 1:
            p.hasuppergap, p.uppergap = 1, int(gap[1])
    return p


class Select:
    """The matches vmatch would print of the lists added (vsa_select): what
    matchokay lets through, the N best of it, sorted.  layout: what
    sink_params() returns; queries: the batch the lists refer to (its lengths
    and offset), or None for the query Multiseq of the layout."""

    def __init__(self, layout, queries=None, device=0, **options):
        self._layout = layout
        p = options.pop("params", None) or select_params(**options)
        self._h = C.c_void_p()
        _check(lib.vsa_select_open(C.byref(layout[0]),
                                   queries._h if queries is not None else None,
                                   C.byref(p), device, C.byref(self._h)))

    def add(self, result, palindromic=False):
        _check(lib.vsa_select_add(self._h, result._h, int(bool(palindromic))))

    def finish(self):
        """-> Result: the selection as raw records in output order"""
        h = C.c_void_p()
        _check(lib.vsa_select_finish(self._h, C.byref(h)))
        return Result(h)

    def flags(self, n):
        """the D/P flags of the n records finish() delivered last"""
        out = np.zeros(n, np.uint8)
        _check(lib.vsa_select_flags(self._h, _ptr(out), n))
        return out

    def stats(self):
        s = SelectStats()
        _check(lib.vsa_select_getstats(self._h, C.byref(s)))
        return s

    @property
    def passes(self):
        """digit-counting passes of the radix select of the last add()"""
        return int(lib.vsa_select_passes(self._h))

    def evalues(self, result, palindromic=False):
        out = np.zeros(result.count, np.float64)
        _check(lib.vsa_select_evalues(self._h, result._h,
                                      int(bool(palindromic)), _ptr(out),
                                      len(out)))
        return out

    def close(self):
        if self._h and lib is not None:
            lib.vsa_select_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def select_host(layout, matches, palindromic=None, **options):
    """the same selection on a list in host memory, no GPU -> (records,
    flags, E-values, SelectStats)"""
    p = options.pop("params", None) or select_params(**options)
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(matches)
    pal = None if palindromic is None else \
        np.ascontiguousarray(palindromic, np.uint8)
    assert pal is None or len(pal) == n
    out = np.zeros(n, MATCH_DTYPE)
    flags, ev = np.zeros(n, np.uint8), np.zeros(n, np.float64)
    k, st = C.c_uint64(0), SelectStats()
    _check(lib.vsa_select_host(C.byref(layout[0]), C.byref(p), _ptr(matches),
                               _ptr(pal), n, _ptr(out), _ptr(flags), _ptr(ev),
                               n, C.byref(k), C.byref(st)))
    k = int(k.value)
    return out[:k], flags[:k], ev[:k], st


# ---- sequence clustering (vmatch -dbcluster percsmall perclarge) ---------------

CLUSTER_SINGLET = 0xFFFFFFFFFFFFFFFF
CLUSTER_MAXROUNDS, CLUSTER_MAXJUMPS = 64, 64


def _format_capacity(numofsequences, inclusters):
    # three lines, a line per cluster size and per cluster, 21 bytes a member
    return 512 + 64 * (numofsequences // 2 + 2) + 22 * (inclusters + 1)


class Cluster:
    """Single-linkage clusters of the sequences of an index from the match
    lists added (vsa_cluster).  layout: what sink_params() returns, kind
    SINK_SELF (or SINK_QUERY with selfpalindromic for lists of vmatch -p IDX
    alone)."""

    def __init__(self, layout, percsmall, perclarge, device=0):
        self._layout = layout
        self.numofsequences = int(layout[0].numofsequences)
        p = ClusterParams(int(percsmall), int(perclarge))
        self._h = C.c_void_p()
        _check(lib.vsa_cluster_open(C.byref(layout[0]), C.byref(p), device,
                                    C.byref(self._h)))

    def add(self, result, palindromic=False):
        _check(lib.vsa_cluster_add(self._h, result._h,
                                   int(bool(palindromic))))

    def finish(self):
        _check(lib.vsa_cluster_finish(self._h))

    def stats(self):
        s = ClusterStats()
        _check(lib.vsa_cluster_getstats(self._h, C.byref(s)))
        return s

    def members(self):
        """-> (clusterstart, members): cluster c is
        members[clusterstart[c]:clusterstart[c + 1]]"""
        s = self.stats()
        start = np.zeros(s.clusters + 1, np.uint64)
        mem = np.zeros(s.inclusters, np.uint64)
        _check(lib.vsa_cluster_members(self._h, _ptr(start), _ptr(mem)))
        return start, mem

    def labels(self):
        out = np.zeros(self.numofsequences, np.uint64)
        _check(lib.vsa_cluster_labels(self._h, _ptr(out)))
        return out

    def edges(self):
        """-> (Result of the accepted records grouped by cluster, D/P flags,
        edgestart)"""
        s = self.stats()
        flags = np.zeros(s.edges, np.uint8)
        start = np.zeros(s.clusters + 1, np.uint64)
        h = C.c_void_p()
        _check(lib.vsa_cluster_edges(self._h, C.byref(h), _ptr(flags),
                                     _ptr(start)))
        return Result(h), flags, start

    def format(self):
        s = self.stats()
        cap = _format_capacity(self.numofsequences, s.inclusters)
        buf = np.empty(cap, np.uint8)
        n = lib.vsa_cluster_format(self._h, _ptr(buf), cap)
        if n < 0:
            raise VsaError(int(n), messagespace())
        return buf[:n].tobytes()

    def times(self):
        """HIP-event ms of all add / finish / edges calls so far"""
        a, f, e = C.c_double(), C.c_double(), C.c_double()
        _check(lib.vsa_cluster_times(self._h, C.byref(a), C.byref(f),
                                     C.byref(e)))
        return a.value, f.value, e.value

    def close(self):
        if self._h and lib is not None:
            lib.vsa_cluster_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def cluster_host(layout, percsmall, perclarge, matches, palindromic=None,
                 text=True):
    """the same clustering of a list in host memory, no GPU -> dict(stats,
    clusterstart, members, labels, edgestart, edgerecord, text)"""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(matches)
    pal = None if palindromic is None else \
        np.ascontiguousarray(palindromic, np.uint8)
    assert pal is None or len(pal) == n
    nseq = int(layout[0].numofsequences)
    p = ClusterParams(int(percsmall), int(perclarge))
    st = ClusterStats()
    cstart = np.zeros(nseq // 2 + 2, np.uint64)
    estart = np.zeros(nseq // 2 + 2, np.uint64)
    mem = np.zeros(nseq, np.uint64)
    lab = np.zeros(nseq, np.uint64)
    erec = np.zeros(n, np.uint64)
    cap = _format_capacity(nseq, nseq) if text else 0
    buf = np.empty(cap, np.uint8) if text else None
    written = C.c_int64(0)
    _check(lib.vsa_cluster_host(C.byref(layout[0]), C.byref(p), _ptr(matches),
                                _ptr(pal), n, C.byref(st), _ptr(cstart),
                                _ptr(mem), _ptr(lab), _ptr(estart),
                                _ptr(erec), _ptr(buf), cap,
                                C.byref(written)))
    k = int(st.clusters)
    return dict(stats=st, clusterstart=cstart[:k + 1],
                members=mem[:int(st.inclusters)], labels=lab,
                edgestart=estart[:k + 1], edgerecord=erec[:int(st.edges)],
                text=buf[:written.value].tobytes() if text else None)


# ---- match clustering (vmatch -pp matchcluster gapsize G | overlap P) ---------

MATCHCLUSTER_GAP, MATCHCLUSTER_OVERLAP, MATCHCLUSTER_ERATE = 0, 1, 2
MATCHCLUSTER_STAGES = ("refs", "sort", "window", "pairs", "forest", "group")


def _matchcluster_params(mode, value):
    return MatchClusterParams(int(mode),
                              int(value) if mode == MATCHCLUSTER_GAP else 0,
                              int(value) if mode != MATCHCLUSTER_GAP else 0)


def _cluster_text_capacity(size, nedges):
    # "# id m" and a match line per member, a "# linked" line per edge
    return 256 + 224 * size + 96 * nedges


def matchcluster_format_host(sink, mode, members, records, m0, m1, values):
    """the bytes of a cluster's match file behind its first line, from the
    members of one cluster with their records and its edges in host memory"""
    members = np.ascontiguousarray(members, np.uint64)
    records = np.ascontiguousarray(records, MATCH_DTYPE)
    m0 = np.ascontiguousarray(m0, np.uint32)
    m1 = np.ascontiguousarray(m1, np.uint32)
    values = np.ascontiguousarray(values, np.uint64)
    assert len(members) == len(records) and len(m0) == len(m1) == len(values)
    cap = _cluster_text_capacity(len(members), len(m0))
    buf = np.empty(cap, np.uint8)
    n = lib.vsa_matchcluster_format_host(
        sink._h, int(mode), _ptr(members), _ptr(records), len(members),
        _ptr(m0), _ptr(m1), _ptr(values), len(m0), _ptr(buf), cap)
    if n < 0:
        raise VsaError(int(n), messagespace())
    return buf[:n].tobytes()


class MatchCluster:
    """Single-linkage clusters of the matches of the lists added, linked by
    gap or by overlap (vsa_matchcluster).  layout: what sink_params()
    returns; mode MATCHCLUSTER_GAP with value = the largest gap, or
    MATCHCLUSTER_OVERLAP with value = the least overlap in percent."""

    def __init__(self, layout, mode, value, device=0):
        self._layout = layout
        self.mode = int(mode)
        p = _matchcluster_params(mode, value)
        self._h = C.c_void_p()
        _check(lib.vsa_matchcluster_open(C.byref(layout[0]), C.byref(p),
                                         device, C.byref(self._h)))

    @classmethod
    def erate(cls, layout, index, errorrate, device=0):
        """matches linked by the edit distance of their substrings
        (vsa_eratecluster_open): at most `errorrate` percent of the
        shorter one.  The text is that of `index`, which the handle keeps."""
        self = cls.__new__(cls)
        self._layout, self._index = layout, index
        self.mode = MATCHCLUSTER_ERATE
        self._h = C.c_void_p()
        _check(lib.vsa_eratecluster_open(
            C.byref(layout[0]), index._h, int(errorrate), device,
            C.byref(self._h)))
        return self

    def add(self, result, palindromic=False):
        _check(lib.vsa_matchcluster_add(self._h, result._h,
                                        int(bool(palindromic))))

    def finish(self):
        _check(lib.vsa_matchcluster_finish(self._h))

    def stats(self):
        s = MatchClusterStats()
        _check(lib.vsa_matchcluster_getstats(self._h, C.byref(s)))
        return s

    def members(self):
        """-> (clusterstart, members): cluster c is
        members[clusterstart[c]:clusterstart[c + 1]], match numbers"""
        s = self.stats()
        start = np.zeros(s.clusters + 1, np.uint64)
        mem = np.zeros(s.inclusters, np.uint64)
        _check(lib.vsa_matchcluster_members(self._h, _ptr(start), _ptr(mem)))
        return start, mem

    def labels(self):
        out = np.zeros(self.stats().matches, np.uint64)
        _check(lib.vsa_matchcluster_labels(self._h, _ptr(out)))
        return out

    def edges(self):
        """-> (edgestart, m0, m1, values): the edges grouped by cluster in
        the reference's order; values are gaps, or the bits of the overlap
        percentages (values.view(np.float64))"""
        s = self.stats()
        start = np.zeros(s.clusters + 1, np.uint64)
        m0 = np.zeros(s.edges, np.uint32)
        m1 = np.zeros(s.edges, np.uint32)
        val = np.zeros(s.edges, np.uint64)
        _check(lib.vsa_matchcluster_edges(self._h, _ptr(start), _ptr(m0),
                                          _ptr(m1), _ptr(val)))
        return start, m0, m1, val

    def records(self):
        """-> (Result of the member matches of all clusters in member order,
        D/P flags)"""
        flags = np.zeros(self.stats().inclusters, np.uint8)
        h = C.c_void_p()
        _check(lib.vsa_matchcluster_records(self._h, C.byref(h),
                                            _ptr(flags)))
        return Result(h), flags

    def format(self):
        s = self.stats()
        cap = 128 + 96 * (s.clusters + 1)
        buf = np.empty(cap, np.uint8)
        n = lib.vsa_matchcluster_format(self._h, _ptr(buf), cap)
        if n < 0:
            raise VsaError(int(n), messagespace())
        return buf[:n].tobytes()

    def format_cluster(self, sink, c, size, nedges):
        """the bytes of PREFIX.size.c.match behind its first line; size and
        nedges of cluster c bound the text"""
        cap = _cluster_text_capacity(int(size), int(nedges))
        buf = np.empty(cap, np.uint8)
        n = lib.vsa_matchcluster_format_cluster(self._h, sink._h, int(c),
                                                _ptr(buf), cap)
        if n < 0:
            raise VsaError(int(n), messagespace())
        return buf[:n].tobytes()

    def times(self):
        """HIP-event ms of all calls so far per stage -> dict"""
        ms = np.zeros(len(MATCHCLUSTER_STAGES), np.float64)
        _check(lib.vsa_matchcluster_times(self._h, _ptr(ms)))
        return dict(zip(MATCHCLUSTER_STAGES, ms.tolist()))

    def close(self):
        if self._h and lib is not None:
            lib.vsa_matchcluster_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def matchcluster_host(layout, mode, value, matches, palindromic=None,
                      text=True):
    """the same clustering of a list in host memory, no GPU -> dict(stats,
    clusterstart, members, labels, edgestart, m0, m1, values, text)"""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(matches)
    pal = None if palindromic is None else \
        np.ascontiguousarray(palindromic, np.uint8)
    assert pal is None or len(pal) == n
    p = _matchcluster_params(mode, value)
    st = MatchClusterStats()
    # once for the number of edges, once for the edges
    _check(lib.vsa_matchcluster_host(C.byref(layout[0]), C.byref(p),
                                     _ptr(matches), _ptr(pal), n,
                                     C.byref(st), None, None, None, None,
                                     None, None, None, 0, None, 0, None))
    ne = int(st.edges)
    cstart = np.zeros(n // 2 + 2, np.uint64)
    estart = np.zeros(n // 2 + 2, np.uint64)
    mem = np.zeros(n, np.uint64)
    lab = np.zeros(n, np.uint64)
    m0 = np.zeros(ne, np.uint32)
    m1 = np.zeros(ne, np.uint32)
    val = np.zeros(ne, np.uint64)
    cap = 128 + 96 * (n // 2 + 2) if text else 0
    buf = np.empty(cap, np.uint8) if text else None
    written = C.c_int64(0)
    _check(lib.vsa_matchcluster_host(C.byref(layout[0]), C.byref(p),
                                     _ptr(matches), _ptr(pal), n,
                                     C.byref(st), _ptr(cstart), _ptr(mem),
                                     _ptr(lab), _ptr(estart), _ptr(m0),
                                     _ptr(m1), _ptr(val), ne, _ptr(buf), cap,
                                     C.byref(written)))
    k = int(st.clusters)
    return dict(stats=st, clusterstart=cstart[:k + 1],
                members=mem[:int(st.inclusters)], labels=lab,
                edgestart=estart[:k + 1], m0=m0, m1=m1, values=val,
                text=buf[:written.value].tobytes() if text else None)


def matchcluster_erate_host(layout, errorrate, text_symbols, matches,
                            text=True, edges=None):
    """vmatch -pp matchcluster erate E on a list and the symbols of the index
    text in host memory, no GPU -> the dict of matchcluster_host; values =
    minlen << 32 | edit distance.  edges: room for that many edges (default
    16 per match).  The work is quadratic in the list: it is done once, and
    once more only where the edges did not fit (-3, which leaves their number
    in the stats)."""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    tis = np.ascontiguousarray(text_symbols, np.uint8)
    n = len(matches)
    st = MatchClusterStats()
    cstart = np.zeros(n // 2 + 2, np.uint64)
    estart = np.zeros(n // 2 + 2, np.uint64)
    mem = np.zeros(n, np.uint64)
    lab = np.zeros(n, np.uint64)
    cap = 128 + 96 * (n // 2 + 2) if text else 0
    buf = np.empty(cap, np.uint8) if text else None
    written = C.c_int64(0)
    room = 16 * n + 1024 if edges is None else int(edges)
    while True:
        m0 = np.zeros(room, np.uint32)
        m1 = np.zeros(room, np.uint32)
        val = np.zeros(room, np.uint64)
        rc = lib.vsa_eratecluster_host(
            C.byref(layout[0]), int(errorrate), _ptr(tis), len(tis),
            _ptr(matches), n, C.byref(st), _ptr(cstart), _ptr(mem), _ptr(lab),
            _ptr(estart), _ptr(m0), _ptr(m1), _ptr(val), room, _ptr(buf), cap,
            C.byref(written))
        if rc != -3 or int(st.edges) <= room:
            break
        room = int(st.edges)
    _check(rc)
    k, ne = int(st.clusters), int(st.edges)
    return dict(stats=st, clusterstart=cstart[:k + 1],
                members=mem[:int(st.inclusters)], labels=lab,
                edgestart=estart[:k + 1], m0=m0[:ne], m1=m1[:ne],
                values=val[:ne],
                text=buf[:written.value].tobytes() if text else None)


# ---- chaining (vmatch -pp chain ...) --------------------------------------------

CHAIN_GLOBAL, CHAIN_GLOBAL_GC, CHAIN_GLOBAL_OV, CHAIN_LOCAL_MAX, \
    CHAIN_LOCAL_THRESHOLD, CHAIN_LOCAL_BEST, CHAIN_LOCAL_PERCENT = range(7)
CHAIN_MAXGROUP = 1 << 15
CHAIN_SILENT = 1
CHAIN_STAGES = ("view", "sort", "replay", "score", "retrieve")


def _chain_params(kind, value, maxgap, wf, withinborders, thread=False):
    return ChainParams(int(kind), int(value), int(maxgap), float(wf),
                       int(bool(withinborders)), int(bool(thread)))


def _chain_text_capacity(chains, chained):
    # a header per chain, a match line per member
    return 256 + 96 * chains + 224 * chained


def chain_format_host(sink, number, score, start, records, silent=False):
    """the reference's text of chains in host memory: records[t] = the
    record of member t of all chains"""
    number = np.ascontiguousarray(number, np.uint64)
    score = np.ascontiguousarray(score, np.int64)
    start = np.ascontiguousarray(start, np.uint64)
    records = np.ascontiguousarray(records, MATCH_DTYPE)
    assert len(number) == len(score) == len(start) - 1
    cap = _chain_text_capacity(len(number), len(records))
    buf = np.empty(cap, np.uint8)
    n = lib.vsa_chain_format_host(sink._h, CHAIN_SILENT if silent else 0,
                                  len(number), _ptr(number), _ptr(score),
                                  _ptr(start), _ptr(records), _ptr(buf), cap)
    if n < 0:
        raise VsaError(int(n), messagespace())
    return buf[:n].tobytes()


class Chain:
    """Chains of the matches of the lists added (vsa_chain): global, with
    gap costs, with overlaps, or local, per sequence pair (withinborders) or
    over the whole list.  layout: what sink_params() returns."""

    def __init__(self, layout, kind=CHAIN_GLOBAL, value=0, maxgap=0, wf=1.0,
                 withinborders=False, thread=False, device=0):
        self._layout = layout
        p = _chain_params(kind, value, maxgap, wf, withinborders, thread)
        self._h = C.c_void_p()
        _check(lib.vsa_chain_open(C.byref(layout[0]), C.byref(p), device,
                                  C.byref(self._h)))

    def add(self, result, palindromic=False):
        _check(lib.vsa_chain_add(self._h, result._h, int(bool(palindromic))))

    def finish(self):
        _check(lib.vsa_chain_finish(self._h))

    def stats(self):
        s = ChainStats()
        _check(lib.vsa_chain_getstats(self._h, C.byref(s)))
        return s

    def chains(self):
        """-> dict(problem, number, score, start, members): chain c has the
        members members[start[c]:start[c + 1]], record numbers"""
        s = self.stats()
        out = dict(problem=np.zeros(s.chains, np.uint64),
                   number=np.zeros(s.chains, np.uint64),
                   score=np.zeros(s.chains, np.int64),
                   start=np.zeros(s.chains + 1, np.uint64),
                   members=np.zeros(s.chained, np.uint64))
        _check(lib.vsa_chain_chains(self._h, _ptr(out["problem"]),
                                    _ptr(out["number"]), _ptr(out["score"]),
                                    _ptr(out["start"])))
        _check(lib.vsa_chain_members(self._h, _ptr(out["members"])))
        return out

    def records(self):
        """-> (Result of the members of all chains in member order, D/P
        flags)"""
        flags = np.zeros(self.stats().chained, np.uint8)
        h = C.c_void_p()
        _check(lib.vsa_chain_records(self._h, C.byref(h), _ptr(flags)))
        return Result(h), flags

    def format(self, sink, silent=False):
        s = self.stats()
        cap = _chain_text_capacity(s.chains, s.chained)
        buf = np.empty(cap, np.uint8)
        n = lib.vsa_chain_format(self._h, sink._h,
                                 CHAIN_SILENT if silent else 0, _ptr(buf),
                                 cap)
        if n < 0:
            raise VsaError(int(n), messagespace())
        return buf[:n].tobytes()

    def times(self):
        """HIP-event ms of all calls so far per stage -> dict"""
        ms = np.zeros(len(CHAIN_STAGES), np.float64)
        _check(lib.vsa_chain_times(self._h, _ptr(ms)))
        return dict(zip(CHAIN_STAGES, ms.tolist()))

    def close(self):
        if self._h and lib is not None:
            lib.vsa_chain_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def chain_host(layout, matches, palindromic=None, kind=CHAIN_GLOBAL, value=0,
               maxgap=0, wf=1.0, withinborders=False, thread=False):
    """the same chaining of a list in host memory, no GPU, problems of any
    size -> dict(stats, problem, number, score, start, members)"""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    n = len(matches)
    pal = None if palindromic is None else \
        np.ascontiguousarray(palindromic, np.uint8)
    assert pal is None or len(pal) == n
    p = _chain_params(kind, value, maxgap, wf, withinborders, thread)
    st = ChainStats()
    # once for the counts, once for the chains
    _check(lib.vsa_chain_host(C.byref(layout[0]), C.byref(p), _ptr(matches),
                              _ptr(pal), n, C.byref(st), None, None, None,
                              None, 0, None, 0))
    k, m = int(st.chains), int(st.chained)
    out = dict(problem=np.zeros(k, np.uint64), number=np.zeros(k, np.uint64),
               score=np.zeros(k, np.int64), start=np.zeros(k + 1, np.uint64),
               members=np.zeros(m, np.uint64))
    _check(lib.vsa_chain_host(C.byref(layout[0]), C.byref(p), _ptr(matches),
                              _ptr(pal), n, C.byref(st),
                              _ptr(out["problem"]), _ptr(out["number"]),
                              _ptr(out["score"]), _ptr(out["start"]), k,
                              _ptr(out["members"]), m))
    out["stats"] = st
    return out


# ---- synthetic inputs ------------------------------

GENOME_SEED = 42
QUERY_SEED = 4242


def synth_genome(n, seed=GENOME_SEED):
    g = np.zeros(n, np.uint8)
    lib.vsa_synth_genome(seed, n, _ptr(g))
    return g


def synth_queries(genome, nq, m, seed=QUERY_SEED):
    genome = np.ascontiguousarray(genome, np.uint8)
    q = np.zeros(nq * m, np.uint8)
    lib.vsa_synth_queries(seed, _ptr(genome), genome.shape[0], nq, m,
                          _ptr(q), None)
    return q


def pack_reads(symbols, nq, m, stride=None, specialcap=None, threads=1):
    """-> (rows u64[nq * W], special u8[ns * m], ns)"""
    stride = m if stride is None else stride
    W = int(lib.vsa_packed_words(m))
    rows = np.zeros(nq * W, np.uint64)
    cap = nq if specialcap is None else specialcap
    special = np.zeros(max(cap, 1) * m, np.uint8)
    ns = C.c_uint64(0)
    _check(lib.vsa_pack_reads_mt(_ptr(symbols), nq, m, stride, _ptr(rows),
                                 _ptr(special), cap, C.byref(ns), threads))
    return rows, special[:ns.value * m], int(ns.value)


def synth_query_plan(n, nq, m, seed=QUERY_SEED):
    pos = np.zeros(nq, np.uint64)
    sub = np.zeros(nq, np.uint32)
    step = np.zeros(nq, np.uint8)
    lib.vsa_synth_query_plan(seed, n, nq, m, _ptr(pos), _ptr(sub),
                             _ptr(step))
    return pos, sub, step


def mkvtree(dbfiles, indexname, queryfiles=(), prefixlength=0, integersize=64,
            withskp=True, device=0):
    """mkvtree -db .. [-q ..] -indexname .. -dna -pl -allout on the GPU."""
    db = (C.c_char_p * len(dbfiles))(*[os.fsencode(f) for f in dbfiles])
    qf = (C.c_char_p * max(1, len(queryfiles)))(
        *[os.fsencode(f) for f in queryfiles])
    _check(lib.vsa_mkvtree(db, len(dbfiles), qf, len(queryfiles),
                           os.fsencode(indexname), prefixlength, integersize,
                           int(withskp), device))


def device_count():
    return int(lib.vsa_device_count())


def device_synchronize(device=0):
    _check(lib.vsa_device_synchronize(device))


def device_malloc(nbytes, device=0):
    p = C.c_void_p()
    _check(lib.vsa_device_malloc(nbytes, device, C.byref(p)))
    return p


def device_upload(dptr, array, device=0):
    array = np.ascontiguousarray(array)
    _check(lib.vsa_device_upload(dptr, _ptr(array), array.nbytes, device))


def device_download(array, dptr, device=0):
    """device memory -> a contiguous numpy array (its size decides)"""
    assert array.flags["C_CONTIGUOUS"]
    _check(lib.vsa_device_download(_ptr(array), dptr, array.nbytes, device))


def device_meminfo(device=0, trim=True):
    """(free, total) bytes of the device, the library's cache handed back"""
    if trim:
        _check(lib.vsa_device_trim(device))
    f, t = C.c_uint64(0), C.c_uint64(0)
    _check(lib.vsa_device_meminfo(device, C.byref(f), C.byref(t)))
    return int(f.value), int(t.value)


def device_free(p, device=0):
    _check(lib.vsa_device_free(p, device))


def measure_stream_read(nbytes=1 << 30, device=0):
    g = C.c_double()
    _check(lib.vsa_measure_stream_read(nbytes, device, C.byref(g)))
    return g.value


# ---- degenerate matches: vmatch -l L -h K [-seedlength S] [-q Q] IDX ---------

HAMMING_LENGTHBITS = 48
HAMMING_MAXDISTANCE = 0xFFFF
# limits of the device path (include/vstree_amd.h); VSA_EXTEND_STAGE=lane|long
# in the environment forces one scan stage
EXTEND_MAXDIST = int(lib.vsa_extend_maxdist())
EXTEND_LANE_BUDGET = int(lib.vsa_extend_lane_budget())
EXTEND_LONG_STEP = int(lib.vsa_extend_long_step())


def hamming_lengths(matches):
    """the lengths of records of extended seeds"""
    return matches["length"] & np.uint64((1 << HAMMING_LENGTHBITS) - 1)


def hamming_distances(matches):
    """... and their numbers of mismatches"""
    return matches["length"] >> np.uint64(HAMMING_LENGTHBITS)


def extend_seedlength(leastlength, maxdist, seedlength=0):
    """max(S, L / (K + 1)), Vmatch/matchlenparm.c:11-22"""
    return int(lib.vsa_extend_seedlength(int(leastlength), int(maxdist),
                                         int(seedlength)))


def _extension(kind, docs, flag=None):
    """the four wrappers of one kind of extension of exact seeds, `kind` as in
    the names of its entries: (extend_KIND, findquerymatches_KIND,
    findselfmatches_KIND, extend_KIND_host) with the docstrings `docs`.
    flag: the name of a keyword argument every wrapper requires, a truth
    value that follows the bound in the entries of the kind"""
    def own(kw):
        if set(kw) != ({flag} if flag else set()):
            raise TypeError("%s: keyword arguments %s" % (
                kind, sorted(kw) if not flag else "need `%s` only" % flag))
        return tuple(int(bool(v)) for v in kw.values())

    c_extend = getattr(lib, "vsa_extend_" + kind)
    c_query = getattr(lib, "vsa_findquerymatches_" + kind)
    c_self = getattr(lib, "vsa_findselfmatches_" + kind)
    c_host = getattr(lib, "vsa_extend_%s_host" % kind)

    def extend(index, queries, seeds, leastlength, maxdist, seedlength=0,
               palindromic=False, **kw):
        p = SinkParams()
        p.kind = SINK_SELF if queries is None else SINK_QUERY
        h = C.c_void_p()
        _check(c_extend(index._h, None if queries is None else queries._h,
                        seeds._h, C.byref(p), int(bool(palindromic)),
                        int(leastlength), int(maxdist), *own(kw),
                        int(seedlength), C.byref(h)))
        return Result(h)

    def findquerymatches(index, queries, leastlength, maxdist, seedlength=0,
                         palindromic=False, **kw):
        h = C.c_void_p()
        _check(c_query(index._h, queries._h, int(leastlength), int(maxdist),
                       *own(kw), int(seedlength), int(bool(palindromic)),
                       C.byref(h)))
        return Result(h)

    def findselfmatches(index, leastlength, maxdist, seedlength=0, **kw):
        h = C.c_void_p()
        _check(c_self(index._h, int(leastlength), int(maxdist), *own(kw),
                      int(seedlength), C.byref(h)))
        return Result(h)

    def extend_host(text, seeds, leastlength, maxdist, seedlength=0,
                    queries=None, numofchars=4, threads=0, **kw):
        text = np.ascontiguousarray(text, np.uint8)
        seeds = np.ascontiguousarray(seeds, MATCH_DTYPE)
        p, keep = sink_params(
            SINK_SELF if queries is None else SINK_QUERY, len(text), (),
            numofchars=numofchars,
            querystart=None if queries is None else queries[1],
            querylength=None if queries is None else queries[2])
        qsym = None if queries is None else np.ascontiguousarray(queries[0],
                                                                 np.uint8)
        out = np.zeros(len(seeds), MATCH_DTYPE)
        n = C.c_uint64()
        _check(c_host(C.byref(p), _ptr(text), _ptr(qsym), _ptr(seeds),
                      len(seeds), int(leastlength), int(maxdist), *own(kw),
                      int(seedlength), int(threads), _ptr(out), len(out),
                      C.byref(n)))
        return out[:n.value]

    made = (extend, findquerymatches, findselfmatches, extend_host)
    for fn, name, doc in zip(made, ("extend_%s", "findquerymatches_%s",
                                    "findselfmatches_%s", "extend_%s_host"),
                             docs):
        fn.__name__ = fn.__qualname__ = name % kind
        fn.__doc__ = doc
    return made


(extend_hamming, findquerymatches_hamming, findselfmatches_hamming,
 extend_hamming_host) = _extension("hamming", (
     """hammingextend (kurtz/extendHD.c:166) for every seed of a Result:
    queries = the forward batch of MEM seeds (palindromic: found on its
    reverse complement), or None for the seeds of findmaximalrepeats""",
     """vmatch -l L -h K [-seedlength S] [-p] -q Q IDX""",
     """vmatch -l L -h K [-seedlength S] IDX""",
     """the same extension on the host, any distance bound: text = the symbols
    of the index, queries = (symbols, start, length) of the batch the seeds
    refer to (for -p: its reverse complement), or None for self seeds"""))


# ---- degenerate matches: vmatch -l L -e K [-seedlength S] [-p] [-q Q] IDX ----
# (include/vstree_amd_edist.h; the record: length1 in bits 0-47 of the length,
# the distance in bits 48-55, length2 - length1 as a signed byte above)

SINK_QUERY_EDIST, SINK_SELF_EDIST = 10, 11
EDIST_MAXDISTANCE = 125
EXTEND_EDIST_MAXDIST = int(lib.vsa_extend_edist_maxdist())


def edist_lengths1(matches):
    return matches["length"] & np.uint64((1 << 48) - 1)


def edist_distances(matches):
    return (matches["length"] >> np.uint64(48)) & np.uint64(0xFF)


def edist_lengths2(matches):
    diff = (matches["length"] >> np.uint64(56)).astype(np.uint8)
    return (edist_lengths1(matches).astype(np.int64) +
            diff.astype(np.int8).astype(np.int64)).astype(np.uint64)


def edist_pack(length1, length2, distance):
    length1 = np.asarray(length1, np.uint64)
    diff = (np.asarray(length2, np.uint64) - length1) & np.uint64(0xFF)
    return (length1 | np.asarray(distance, np.uint64) << np.uint64(48) |
            diff << np.uint64(56))


(extend_edist, findquerymatches_edist, findselfmatches_edist,
 extend_edist_host) = _extension("edist", (
     """editextend (kurtz/extendED.c:78) for every seed of a Result; arguments
    as for extend_hamming""",
     """vmatch -l L -e K [-seedlength S] [-p] -q Q IDX""",
     """vmatch -l L -e K [-seedlength S] IDX""",
     """the same extension on the host, any distance bound the record carries;
    arguments as for extend_hamming_host"""))


# ---- X-drop extension: vmatch -l L -hxdrop X | -exdrop X [-seedlength S] -----
# (include/vstree_amd_xdrop.h; the record: length1 in bits 0-31 of the length,
# length2 above; the start in the query sequence in bits 0-31 of querystart,
# the magnitude of the distance above -- negative for -hxdrop)

SINK_QUERY_HXDROP, SINK_SELF_HXDROP, SINK_QUERY_EXDROP, SINK_SELF_EXDROP = \
    12, 13, 14, 15
XDROP_MAXDROP = 255


def xdrop_lengths1(matches):
    return matches["length"] & np.uint64(0xFFFFFFFF)


def xdrop_lengths2(matches):
    return matches["length"] >> np.uint64(32)


def xdrop_starts(matches):
    return matches["querystart"] & np.uint64(0xFFFFFFFF)


def xdrop_distances(matches):
    """the magnitudes; the kind gives the sign"""
    return matches["querystart"] >> np.uint64(32)


def extend_xdrop_seedlength(seedlength=0):
    """S, or 30 (Vmatch/matchlenparm.c:40-46)"""
    return int(lib.vsa_extend_xdrop_seedlength(int(seedlength)))


(extend_xdrop, findquerymatches_xdrop, findselfmatches_xdrop,
 extend_xdrop_host) = _extension("xdrop", (
     """xdropseedextend (Vmengine/xdropext.c:39) for every seed of a Result;
    arguments as for extend_hamming with X for the bound, and hamming=True
    for -hxdrop, False for -exdrop""",
     """vmatch -l L -hxdrop X | -exdrop X [-seedlength S] [-p] -q Q IDX""",
     """vmatch -l L -hxdrop X | -exdrop X [-seedlength S] IDX""",
     """the same extension on the host; arguments as for extend_hamming_host
    and hamming as above"""), flag="hamming")


# ---- alignments: vmatch -s [W] ------------------------------------------------
# (include/vstree_amd_align.h; a script: 16-bit words, last operation first)

ALIGN_MAXRUN, ALIGN_DELETION, ALIGN_INSERTION, ALIGN_MISMATCH = (
    16383, 0x4000, 0x8000, 0xC000)
ALIGN_MAXDIST = int(lib.vsa_align_maxdist())


class Alignments:
    """The edit scripts of a match list, resident in HBM (vsa_alignments)."""

    def __init__(self, handle):
        self._h = handle

    def stats(self):
        s = AlignStats()
        _check(lib.vsa_alignments_info(self._h, C.byref(s)))
        return s

    def fetch(self):
        """-> (offsets[count + 1], words): the script of record i is
        words[offsets[i]:offsets[i + 1]]"""
        s = self.stats()
        offsets = np.zeros(s.count + 1, np.uint64)
        words = np.zeros(s.words, np.uint16)
        _check(lib.vsa_alignments_fetch(self._h, _ptr(offsets), _ptr(words)))
        return offsets, words

    def close(self):
        if self._h and lib is not None:
            lib.vsa_alignments_free(self._h)
            self._h = None

    def __del__(self):
        self.close()


def align(index, queries, matches, kind, palindromic=False):
    """the scripts of a Result whose records have the layout `kind`
    (SINK_...); queries: the forward batch, or None for a self kind"""
    p = SinkParams()
    p.kind = int(kind)
    h = C.c_void_p()
    _check(lib.vsa_align(index._h, None if queries is None else queries._h,
                         matches._h, C.byref(p), int(bool(palindromic)),
                         C.byref(h)))
    return Alignments(h)


def align_host(kind, text, matches, queries=None, palindromic=False,
               threads=0):
    """the same scripts on the host, any distance a record carries: text = the
    symbols of the index, queries = (symbols, start, length) of the forward
    batch, or None for a self kind -> (offsets, words)"""
    text = np.ascontiguousarray(text, np.uint8)
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    p, keep = sink_params(
        kind, len(text), (),
        querystart=None if queries is None else queries[1],
        querylength=None if queries is None else queries[2])
    qsym = None if queries is None else np.ascontiguousarray(queries[0],
                                                             np.uint8)
    offsets = np.zeros(len(matches) + 1, np.uint64)
    args = (C.byref(p), _ptr(text), _ptr(qsym), _ptr(matches), len(matches),
            int(bool(palindromic)), int(threads), _ptr(offsets))
    # the offsets come with the refusal of a buffer that is too small
    words = np.zeros(16 * len(matches) + 16, np.uint16)
    rc = lib.vsa_align_host(*args, _ptr(words), len(words))
    if rc == -3:
        words = np.zeros(int(offsets[-1]), np.uint16)
        rc = lib.vsa_align_host(*args, _ptr(words), len(words))
    _check(rc)
    return offsets, words[:int(offsets[-1])]


def align_format(sink, matches, offsets, words, text, origtext, queries=None,
                 queryorig=None, linewidth=0):
    """the match lines of `sink` (a Sink) with what vmatch -s W prints behind
    each: origtext / queryorig are the original characters of text /
    queries[0] -> bytes"""
    matches = np.ascontiguousarray(matches, MATCH_DTYPE)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    words = np.ascontiguousarray(words, np.uint16)
    text = np.ascontiguousarray(text, np.uint8)
    origtext = np.ascontiguousarray(origtext, np.uint8)
    qsym = None if queries is None else np.ascontiguousarray(queries[0],
                                                             np.uint8)
    qorig = None if queryorig is None else np.ascontiguousarray(queryorig,
                                                                np.uint8)
    assert len(offsets) == len(matches) + 1
    width = int(linewidth) or 60
    columns = int(offsets[-1]) + 2 * len(matches)
    if len(words):
        runs = words[(words & np.uint16(0xC000)) == 0]
        columns += int(runs.sum(dtype=np.uint64))
    cap = 192 * (len(matches) + 1) + 3 * columns + \
        (3 * (width + 40) + 2) * (columns // width + len(matches) + 1)
    buf = np.empty(cap, np.uint8)
    n = lib.vsa_align_format(sink._h, _ptr(matches), len(matches),
                             _ptr(offsets), _ptr(words), _ptr(text),
                             _ptr(origtext), _ptr(qsym), _ptr(qorig),
                             int(linewidth), _ptr(buf), cap)
    if n < 0:
        raise VsaError(int(n), messagespace())
    return buf[:n].tobytes()


# ---- the scan without an index: vmatch -online -complete --------------------
# (include/vstree_amd_online.h)

ONLINE_EXACT, ONLINE_EDIST, ONLINE_HAMMING = 0, 1, 2
ONLINE_TILE_DEFAULT = 296


class Text:
    """The mapped text alone in one GPU's HBM (vsa_text): what vmatch -online
    maps, TISTAB."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, tis, numofchars=4, device=0):
        tis = np.ascontiguousarray(tis, np.uint8)
        h = C.c_void_p()
        _check(lib.vsa_text_from_host(_ptr(tis), tis.shape[0], numofchars,
                                      device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, device_tis, totallength, numofchars=4, device=0):
        h = C.c_void_p()
        _check(lib.vsa_text_from_device(device_tis, int(totallength),
                                        numofchars, device, C.byref(h)))
        return cls(h)

    @classmethod
    def open(cls, indexname, device=0):
        """NAME.prj, NAME.al1 and NAME.tis (vsa_text_open)"""
        h = C.c_void_p()
        _check(lib.vsa_text_open(os.fsencode(indexname), device, C.byref(h)))
        return cls(h)

    def close(self):
        if self._h and lib is not None:
            lib.vsa_text_close(self._h)
            self._h = None

    def __del__(self):
        self.close()


def findcompletematches_online(where, queries, mode=ONLINE_EXACT, distvalue=0,
                               percent=False, removeredundant=False):
    """vmatch -online -complete [remred] [-e K | -h K] -q: the scan of the
    text of an Index or of a Text.  mode: ONLINE_EXACT, ONLINE_EDIST (-e),
    ONLINE_HAMMING (-h); the distance of a match travels in its querystart
    field.  VsaError.code == NOT_COVERED: left to the CPU reference."""
    fn = (lib.vsa_text_findcompletematches_online if isinstance(where, Text)
          else lib.vsa_findcompletematches_online)
    h = C.c_void_p()
    rc = fn(where._h, queries._h, int(mode), int(distvalue), int(percent),
            int(bool(removeredundant)), C.byref(h))
    assert rc == 0 or not h, "a refusal delivers nothing"
    _check(rc)
    return Result(h)


ONLINE_COUNTERS_DEFAULT = 1 << 26


class OnlinePlan(tuple):
    """(tile, ntiles, queries_per_chunk, numofchunks) of vsa_online_plan"""
    tile = property(lambda s: s[0])
    ntiles = property(lambda s: s[1])
    queries_per_chunk = property(lambda s: s[2])
    numofchunks = property(lambda s: s[3])


def online_plan(totallength, numofqueries, mode=ONLINE_EXACT):
    """how findcompletematches_online cuts a text and a batch
    (vsa_online_plan; a test hook, no GPU needed): symbols or start positions
    per tile, tiles of the text, queries per chunk, chunks -- with
    VSA_ONLINE_TILE and VSA_ONLINE_COUNTERS as the environment has them."""
    tile = C.c_uint32(0)
    out = [C.c_uint64(0) for _ in range(3)]
    _check(lib.vsa_online_plan(int(totallength), int(numofqueries), int(mode),
                               C.byref(tile), *[C.byref(x) for x in out]))
    return OnlinePlan([int(tile.value)] + [int(x.value) for x in out])


def findcompletematches_online_host(tis, symbols, start, length,
                                    mode=ONLINE_EXACT, distvalue=0,
                                    percent=False, removeredundant=False,
                                    offset=0, threads=0, capacity=None):
    """the same on the host (vsa_findcompletematches_online_host): query i is
    symbols[start[i] : start[i] + length[i]] -> MATCH_DTYPE array.  The
    capacity doubles until the list fits unless one is given."""
    tis = np.ascontiguousarray(tis, np.uint8)
    symbols = np.ascontiguousarray(symbols, np.uint8)
    start = np.ascontiguousarray(start, np.uint64)
    length = np.ascontiguousarray(length, np.uint64)
    cap = 1 << 16 if capacity is None else int(capacity)
    while True:
        out = np.zeros(cap, MATCH_DTYPE)
        n = C.c_uint64(0)
        rc = lib.vsa_findcompletematches_online_host(
            _ptr(tis), tis.shape[0], _ptr(symbols), _ptr(start), _ptr(length),
            start.shape[0], int(offset), int(mode), int(distvalue),
            int(percent), int(bool(removeredundant)), int(threads),
            _ptr(out), cap, C.byref(n))
        if rc == -3 and capacity is None:
            cap *= 4
            continue
        _check(rc)
        return out[:n.value].copy()
