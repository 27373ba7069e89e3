"""ctypes view of include/microasm.h (structs + output buffer allocation).

Used by bench.py and tests/ to drive the product library (libmicroasm.so) and -- in tests only --
the oracle (oracle/liboracle.so exports the same layouts with an ``orc_`` prefix).  This module
contains NO compute: it only describes memory.
"""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MA_LIB") or os.path.join(REPO, "lancet2_amd", "libmicroasm.so")  # MA_LIB: developer A/B builds

MA_RF_PASS, MA_RF_CASE, MA_RF_REV = 1, 2, 4
MA_W_NO_HAPLOTYPE, MA_W_HAP_OVERFLOW, MA_W_LEN_OVERFLOW = 1, 2, 4
MA_W_BFS_LIMIT, MA_W_TABLE_OVERFLOW, MA_W_VAR_OVERFLOW = 8, 16, 32
MA_W_CIGAR_OVERFLOW, MA_W_READ_OVERFLOW = 64, 128
MA_MEM_HOST, MA_MEM_DEVICE = 0, 1
MA_NO_HINT = -(1 << 31)


class Params(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "min_k", "max_k", "k_step", "min_node_cov", "min_anchor_cov", "num_samples",
        "min_anchor_len", "max_mismatch", "bfs_limit", "aln_tier", "min_aln_score",
        "max_comps", "max_haps", "max_hap_len", "max_runs", "max_vars", "max_alts",
        "max_allele_bytes", "max_cigar", "case_ctrl_mode")]


def default_params(**kw):
    p = Params(13, 127, 6, 2, 5, 2, 150, 2, 1 << 20, 0, 80, 4, 16, 2048, 256, 64, 4, 4096, 16, 1)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Batch(C.Structure):
    _fields_ = [("n_windows", C.c_int32), ("n_reads", C.c_int64),
                ("ref_bases", C.c_void_p), ("ref_off", C.c_void_p), ("read_win_off", C.c_void_p),
                ("read_off", C.c_void_p), ("read_bases", C.c_void_p), ("read_quals", C.c_void_p),
                ("read_qname_id", C.c_void_p), ("read_sample", C.c_void_p), ("read_flags", C.c_void_p),
                ("read_hint", C.c_void_p)]


class GateOut(C.Structure):
    _fields_ = [("max_approx", C.c_void_p), ("max_exact", C.c_void_p)]


class AsmOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "win_status", "win_k", "win_ncomp", "comp_anchor", "comp_hap0", "comp_nhaps", "comp_cx",
        "comp_cxf", "hap_len", "hap_nruns", "hap_stats", "hap_bases", "hap_runs")]


class VarOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "win_nvars", "var_comp", "var_pos", "var_ref_start", "var_ref_off", "var_ref_len",
        "var_nalts", "alt_off", "alt_len", "alt_type", "alt_length", "var_hap_allele",
        "var_hap_start", "allele_pool")]


class GenoOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "allele_counts", "var_qual", "aln_rec", "aln_cigar", "asg_allele", "asg_score", "var_pl", "var_gq")]


class FmtOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ev_sums", "fmt_npbq", "fmt_cmlod", "fmt_stat")]


MA_RM_SOFTCLIP, MA_RM_PROPER = 1, 2


class ReadMeta(C.Structure):
    """ma_read_meta_t: four per-read arrays, all required"""
    _fields_ = [(n, C.c_void_p) for n in ("read_mapq", "read_mflags", "read_isize", "read_start")]


class FmtMetaOut(C.Structure):
    """ma_fmt_meta_out_t"""
    _fields_ = [(n, C.c_void_p) for n in ("ev_meta", "ev_rpcd", "fmt_rmq", "fmt_mstat")]


META_DTYPES = dict(read_mapq=np.uint8, read_mflags=np.uint8, read_isize=np.int32, read_start=np.int32)


class PackedReads(C.Structure):
    """ma_packed_reads_t"""
    _fields_ = [("bases4", C.c_void_p), ("quals", C.c_void_p), ("qual_bits", C.c_int32), ("qual_dict", C.c_uint8 * 16)]


BASE_CODES = "=ACMGRSVTWYHKDBN"  # BAM's 4-bit base codes


def load_cdll(path=None):
    """dlopen the product library.  PyTorch's ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, no
    SONAME), libmicroasm.so is linked against the system one: whichever of the two initialises second in a process
    finds no device.  Preloading torch's runtime globally (when torch is installed; torch itself is NOT imported) makes
    both resolve to the same runtime whatever the import order."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is not None and spec.submodule_search_locations:
            hip = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(hip):
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
    except Exception:  # no torch, or its runtime cannot be loaded here (CPU-only container): use the system runtime
        pass
    return C.CDLL(path or LIB_PATH)


class CxOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("seq_cx_i", "seq_cx_f", "seq_cx_d", "graph_cx")]


# ma_process_cx_batch(ctx, batch, packed, meta, gate, asm, var, geno, fmt, fmeta, double gc_frac, cx)
PROCESS_CX_ARGTYPES = [C.c_void_p] * 10 + [C.c_double, C.c_void_p]
# ma_set_poa_retry(ctx, int on) / ma_last_poa_retry(ctx, unsigned long long* out, int cap)
SET_POA_RETRY_ARGTYPES = [C.c_void_p, C.c_int]
LAST_POA_RETRY_ARGTYPES = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
POA_RETRY_KEYS = ("marked_width", "marked_capacity", "called", "left_flagged")


BATCH_DTYPES = dict(ref_bases=np.uint8, ref_off=np.uint32, read_win_off=np.uint32,
                    read_off=np.uint64, read_bases=np.uint8, read_quals=np.uint8,
                    read_qname_id=np.uint32, read_sample=np.uint8, read_flags=np.uint8, read_hint=np.int32)


def asm_out_spec(p, n):
    MC, MH, ML, MR = p.max_comps, p.max_haps, p.max_hap_len, p.max_runs
    return dict(win_status=(np.uint32, n), win_k=(np.uint32, n), win_ncomp=(np.uint32, n),
                comp_anchor=(np.uint32, n * MC), comp_hap0=(np.uint32, n * MC),
                comp_nhaps=(np.uint32, n * MC), comp_cx=(np.uint32, n * MC * 3),
                comp_cxf=(np.float64, n * MC * 4), hap_len=(np.uint32, n * MH),
                hap_nruns=(np.uint32, n * MH), hap_stats=(np.float64, n * MH * 6),
                hap_bases=(np.uint8, n * MH * ML), hap_runs=(np.uint32, n * MH * MR * 2))


def var_out_spec(p, n):
    MH, MV, MA, MP = p.max_haps, p.max_vars, p.max_alts, p.max_allele_bytes
    return dict(win_nvars=(np.uint32, n), var_comp=(np.uint32, n * MV), var_pos=(np.uint32, n * MV),
                var_ref_start=(np.uint32, n * MV), var_ref_off=(np.uint32, n * MV),
                var_ref_len=(np.uint32, n * MV), var_nalts=(np.uint32, n * MV),
                alt_off=(np.uint32, n * MV * MA), alt_len=(np.uint32, n * MV * MA),
                alt_type=(np.int32, n * MV * MA), alt_length=(np.int32, n * MV * MA),
                var_hap_allele=(np.uint8, n * MV * MH), var_hap_start=(np.uint32, n * MV * MH),
                allele_pool=(np.uint8, n * MP))


def geno_out_spec(p, n, n_reads, debug=True):
    MH, MV, MA, S, MCG = p.max_haps, p.max_vars, p.max_alts, p.num_samples, p.max_cigar
    spec = dict(allele_counts=(np.uint32, n * MV * S * (MA + 1) * 2), var_qual=(np.float64, n * MV),
                var_pl=(np.uint32, n * MV * S * ((MA + 1) * (MA + 2) // 2)), var_gq=(np.uint32, n * MV * S))
    if debug:
        spec.update(aln_rec=(np.int32, n_reads * MH * 6), aln_cigar=(np.uint32, n_reads * MH * (1 + MCG)),
                    asg_allele=(np.uint8, n_reads * MV), asg_score=(np.float64, n_reads * MV))
    return spec


def fmt_out_spec(p, n):
    """read-level FORMAT statistics (ma_genotype_stats_batch / ma_process_stats_batch); fmt_stat: BQCD, ASMD, AHDD, HSE"""
    MV, MA, S = p.max_vars, p.max_alts, p.num_samples
    return dict(ev_sums=(np.uint32, n * MV * S * (MA + 1) * 3), fmt_npbq=(np.float64, n * MV * S * (MA + 1)),
                fmt_cmlod=(np.float64, n * MV * S * MA), fmt_stat=(np.float64, n * MV * S * 4))


def fmt_meta_out_spec(p, n):
    """the statistics over the read metadata (ma_genotype_meta_batch / ma_process_meta_batch); ev_meta per allele: sum of
    mapq^2, soft-clipped reads, proper pairs with an insert size, sum of their insert sizes; ev_rpcd: n_ref, n_alt, 2 x the ALT
    mid-rank sum, tie term; fmt_mstat: SCA, FLD, RPCD, MQCD, FSSE"""
    MV, MA, S = p.max_vars, p.max_alts, p.num_samples
    return dict(ev_meta=(np.int64, n * MV * S * (MA + 1) * 4), ev_rpcd=(np.uint64, n * MV * S * 4),
                fmt_rmq=(np.float64, n * MV * S * (MA + 1)), fmt_mstat=(np.float64, n * MV * S * 5))


def cx_out_spec(p, n):
    MV = p.max_vars
    return dict(seq_cx_i=(np.int32, n * MV * 4), seq_cx_f=(np.float32, n * MV * 4),
                seq_cx_d=(np.float64, n * MV * 3), graph_cx=(np.float64, n * MV * 3))


MA_G_NODE_OVERFLOW, MA_G_EDGE_OVERFLOW, MA_G_SEQ_OVERFLOW = 1, 2, 4
GRAPH_EXPORT_KEYS = ("tail_small", "tail_large", "tail_hbm", "clean")  # ma_last_graph_export: windows exported per route
GRAPH_LABEL_REFERENCE = 1  # node_label bit 0 (bit 1: CTRL read, bit 2: CASE read)


class GraphOut(C.Structure):
    """ma_graph_out_t: the three caps, then fifteen arrays -- all required"""
    _fields_ = [(n, C.c_int32) for n in ("max_nodes", "max_edges", "max_seq_bytes")] + [(n, C.c_void_p) for n in (
        "win_gstatus", "win_nnodes", "win_nedges", "win_nseq", "node_comp", "node_seq_off", "node_len", "node_cnt",
        "node_sign", "node_label", "node_flags", "edge_src", "edge_dst", "edge_kind", "seq_pool")]


def graph_out_spec(p, n, max_nodes, max_edges, max_seq_bytes):
    """arrays of ma_graph_out_t for n windows at the given per-window caps (ma_assemble_graph_batch)"""
    S, MN, ME, MS = p.num_samples, max_nodes, max_edges, max_seq_bytes
    return dict(win_gstatus=(np.uint32, n), win_nnodes=(np.uint32, n), win_nedges=(np.uint32, n), win_nseq=(np.uint32, n),
                node_comp=(np.uint32, n * MN), node_seq_off=(np.uint32, n * MN), node_len=(np.uint32, n * MN),
                node_cnt=(np.uint32, n * MN * S), node_sign=(np.uint8, n * MN), node_label=(np.uint8, n * MN),
                node_flags=(np.uint8, n * MN), edge_src=(np.uint32, n * ME), edge_dst=(np.uint32, n * ME),
                edge_kind=(np.uint8, n * ME), seq_pool=(np.uint8, n * MS))


def make_graph_struct(arrays, max_nodes, max_edges, max_seq_bytes):
    """ma_graph_out_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller)"""
    s = fill_struct(GraphOut, {k: v for k, v in arrays.items() if k not in ("max_nodes", "max_edges", "max_seq_bytes")})
    s.max_nodes, s.max_edges, s.max_seq_bytes = int(max_nodes), int(max_edges), int(max_seq_bytes)
    return s


MA_ERR_ARG, MA_ERR_PARAM = -1, -5
PROBE_MAX_PER_WINDOW, PROBE_MAX_ALLELE = 256, 256
PROBE_DTYPES = dict(probe_win_off=np.uint32, probe_pos=np.uint32, probe_ref_len=np.uint32, probe_alt_off=np.uint32,
                    probe_alt_len=np.uint32, alt_pool=np.uint8)


class Probes(C.Structure):
    """ma_probes_t: six arrays, all required"""
    _fields_ = [(n, C.c_void_p) for n in PROBE_DTYPES]


class ProbeOut(C.Structure):
    """ma_probe_out_t: six arrays indexed by probe, all required"""
    _fields_ = [(n, C.c_void_p) for n in ("pb_k", "pb_alt_kmers", "pb_in_reads", "pb_lowcov1", "pb_final", "pb_hap_mask")]


def probe_out_spec(p, n_probes):
    """arrays of ma_probe_out_t for n_probes probes (ma_assemble_probe_batch); profiles are count, edge, interior, gaps"""
    P, MC = n_probes, p.max_comps
    return dict(pb_k=(np.uint32, P), pb_alt_kmers=(np.uint32, P), pb_in_reads=(np.uint32, P * 2), pb_lowcov1=(np.uint32, P * 4),
                pb_final=(np.uint32, P * MC * 4), pb_hap_mask=(np.uint32, P * MC))


def pack_probes(per_window):
    """ma_probes_t's arrays from one list of (pos, ref_len, alt bytes) per window, in window order"""
    win_off, pos, ref_len, alt_off, alt_len, pool = [0], [], [], [], [], bytearray()
    for probes in per_window:
        for p, rl, alt in probes:
            pos.append(p)
            ref_len.append(rl)
            alt_off.append(len(pool))
            alt_len.append(len(alt))
            pool += bytes(alt)
        win_off.append(len(pos))
    u32 = lambda v: np.asarray(v, dtype=np.uint32)  # noqa: E731
    return dict(probe_win_off=u32(win_off), probe_pos=u32(pos), probe_ref_len=u32(ref_len), probe_alt_off=u32(alt_off),
                probe_alt_len=u32(alt_len), alt_pool=np.frombuffer(bytes(pool) + b"\0", dtype=np.uint8).copy())


MA_P_NODE_OVERFLOW, MA_P_EDGE_OVERFLOW, MA_P_COL_OVERFLOW = 1, 2, 4
POA_EXPORT_KEYS = ("first", "lab32", "retry_width", "retry_capacity")  # ma_last_poa_export: windows exported per kind of pass
POA_OUT_CAPS = ("max_pnodes", "max_pedges", "max_cols")


class PoaOut(C.Structure):
    """ma_poa_out_t: the three caps, then eighteen arrays -- all required"""
    _fields_ = [(n, C.c_int32) for n in POA_OUT_CAPS] + [(n, C.c_void_p) for n in (
        "win_pstatus", "win_npnodes", "win_npedges", "win_ncols", "comp_pnode0", "comp_npnodes", "comp_pedge0", "comp_npedges",
        "comp_ncols", "pnode_base", "pnode_rank", "pnode_col", "pnode_haps", "pedge_tail", "pedge_head", "pedge_haps",
        "hap_first", "msa")]


def poa_out_spec(p, n, max_pnodes, max_pedges, max_cols):
    """arrays of ma_poa_out_t for n windows: max_pnodes / max_pedges per window, max_cols per component (ma_msa_graph_batch)"""
    MC, MH, MN, ME, MX = p.max_comps, p.max_haps, max_pnodes, max_pedges, max_cols
    return dict(win_pstatus=(np.uint32, n), win_npnodes=(np.uint32, n), win_npedges=(np.uint32, n), win_ncols=(np.uint32, n),
                comp_pnode0=(np.uint32, n * MC), comp_npnodes=(np.uint32, n * MC), comp_pedge0=(np.uint32, n * MC),
                comp_npedges=(np.uint32, n * MC), comp_ncols=(np.uint32, n * MC), pnode_base=(np.uint8, n * MN),
                pnode_rank=(np.uint32, n * MN), pnode_col=(np.uint32, n * MN), pnode_haps=(np.uint32, n * MN),
                pedge_tail=(np.uint32, n * ME), pedge_head=(np.uint32, n * ME), pedge_haps=(np.uint32, n * ME),
                hap_first=(np.uint32, n * MH), msa=(np.uint8, n * MH * MX))


def make_poa_struct(arrays, max_pnodes, max_pedges, max_cols):
    """ma_poa_out_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller)"""
    s = fill_struct(PoaOut, {k: v for k, v in arrays.items() if k not in POA_OUT_CAPS})
    s.max_pnodes, s.max_pedges, s.max_cols = int(max_pnodes), int(max_pedges), int(max_cols)
    return s


FLATTEN_MAX_WINDOW = 16384  # MA_FLATTEN_MAX_WINDOW: records per window that ma_flatten_records_batch sorts
RECORDS_DTYPES = dict(blob=np.uint8, rec_off=np.uint64, rec_len=np.uint32, rec_win_off=np.uint32, rec_sample=np.uint8,
                      sample_index=np.uint8, sample_case=np.uint8, sample_rank=np.uint32, ref_map=np.int32,
                      win_chrom=np.int32, win_start0=np.int64)


class Records(C.Structure):
    """ma_records_t: raw BAM alignment records and which window each belongs to; ref_map may be NULL (identity)"""
    _fields_ = [("n_windows", C.c_int32), ("n_records", C.c_int64), ("blob", C.c_void_p), ("blob_bytes", C.c_uint64),
                ("rec_off", C.c_void_p), ("rec_len", C.c_void_p), ("rec_win_off", C.c_void_p), ("rec_sample", C.c_void_p),
                ("n_samples_in", C.c_int32), ("sample_index", C.c_void_p), ("sample_case", C.c_void_p),
                ("sample_rank", C.c_void_p), ("n_refs", C.c_int32), ("ref_map", C.c_void_p), ("win_chrom", C.c_void_p),
                ("win_start0", C.c_void_p)]


class FlatOut(C.Structure):
    """ma_flat_out_t: the capacity, then thirteen arrays -- all required"""
    _fields_ = [("bases_cap", C.c_uint64)] + [(n, C.c_void_p) for n in (
        "n_bases", "read_off", "bases4", "read_quals", "read_qname_id", "read_sample", "read_flags", "read_hint", "read_mapq",
        "read_mflags", "read_isize", "read_start", "read_src")]


def flat_out_spec(n_records, bases_cap):
    """arrays of ma_flat_out_t for n_records records and room for bases_cap bases (ma_flatten_records_batch)"""
    n, B = int(n_records), int(bases_cap)
    return dict(n_bases=(np.uint64, 1), read_off=(np.uint64, n + 1), bases4=(np.uint8, (B + n + 1) // 2),
                read_quals=(np.uint8, B), read_qname_id=(np.uint32, n), read_sample=(np.uint8, n), read_flags=(np.uint8, n),
                read_hint=(np.int32, n), read_mapq=(np.uint8, n), read_mflags=(np.uint8, n), read_isize=(np.int32, n),
                read_start=(np.int32, n), read_src=(np.uint32, n))


def records_spec(n_windows, n_records, blob_bytes, n_samples_in, n_refs=0):
    """arrays of ma_records_t (ref_map only with n_refs > 0)"""
    n, r, s = int(n_windows), int(n_records), int(n_samples_in)
    spec = dict(blob=(np.uint8, int(blob_bytes)), rec_off=(np.uint64, r), rec_len=(np.uint32, r), rec_win_off=(np.uint32, n + 1),
                rec_sample=(np.uint8, r), sample_index=(np.uint8, s), sample_case=(np.uint8, s), sample_rank=(np.uint32, s),
                win_chrom=(np.int32, n), win_start0=(np.int64, n))
    if n_refs > 0:
        spec["ref_map"] = (np.int32, s * int(n_refs))
    return spec


def make_records_struct(arrays, n_windows, n_records, n_refs=0, blob_bytes=None):
    """ma_records_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller).  The counts that
    are not arguments come from the arrays where those are numpy: blob_bytes = len(blob), n_samples_in = len(sample_rank)
    (or arrays['n_samples_in'])."""
    s = fill_struct(Records, {k: v for k, v in arrays.items() if k in RECORDS_DTYPES})
    s.n_windows, s.n_records, s.n_refs = int(n_windows), int(n_records), int(n_refs)
    s.blob_bytes = int(blob_bytes if blob_bytes is not None else arrays["blob_bytes"] if "blob_bytes" in arrays else len(arrays["blob"]))
    s.n_samples_in = int(arrays["n_samples_in"] if "n_samples_in" in arrays else len(arrays["sample_rank"]))
    return s


def make_flat_struct(arrays, bases_cap):
    """ma_flat_out_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller)"""
    s = fill_struct(FlatOut, {k: v for k, v in arrays.items() if k != "bases_cap"})
    s.bases_cap = int(bases_cap)
    return s


MA_SK_COLLECT, MA_SK_ELIGIBLE = 1, 2
MA_S_ACTIVE, MA_S_LOW_COVERAGE, MA_S_CAPPED, MA_S_MD_RANGE, MA_S_EVENTS, MA_S_LISTED = 1, 2, 4, 8, 16, 32
MA_S_HOST_BITS = MA_S_CAPPED | MA_S_MD_RANGE | MA_S_EVENTS
SELECT_EVENT_KEYS = 8192  # MA_SELECT_EVENT_KEYS: distinct (multiset, position) keys of one (window, sample)
SELECT_IN_KEYS = ("blob", "rec_off", "rec_len", "rec_win_off", "rec_sample")  # what ma_select_records_batch reads of ma_records_t


class SelectParams(C.Structure):
    """ma_select_params_t"""
    _fields_ = [("max_sample_cov", C.c_double), ("min_anchor_cov", C.c_uint32), ("skip_active_region", C.c_int32),
                ("win_len", C.c_void_p)]


class SelectOut(C.Structure):
    """ma_select_out_t: ten arrays -- all required"""
    _fields_ = [(n, C.c_void_p) for n in ("rec_keep", "win_state", "win_sample_reads", "win_sample_bases", "n_selected",
                                          "sel_win_off", "sel_off", "sel_len", "sel_sample", "sel_src")]


def select_out_spec(n_windows, n_records, n_samples_in):
    """arrays of ma_select_out_t (ma_select_records_batch)"""
    n, r, s = int(n_windows), int(n_records), int(n_samples_in)
    return dict(rec_keep=(np.uint8, r), win_state=(np.uint8, n), win_sample_reads=(np.uint32, n * s),
                win_sample_bases=(np.uint64, n * s), n_selected=(np.uint64, 1), sel_win_off=(np.uint32, n + 1),
                sel_off=(np.uint64, r), sel_len=(np.uint32, r), sel_sample=(np.uint8, r), sel_src=(np.uint32, r))


def make_select_params(win_len, max_sample_cov=1000.0, min_anchor_cov=5, skip_active_region=False):
    """ma_select_params_t; win_len: a numpy array, a torch tensor or a raw pointer (kept alive by the caller)"""
    s = fill_struct(SelectParams, dict(win_len=win_len))
    s.max_sample_cov, s.min_anchor_cov, s.skip_active_region = float(max_sample_cov), int(min_anchor_cov), int(bool(skip_active_region))
    return s


MA_Z_HEADER, MA_Z_ISIZE, MA_Z_DATA, MA_Z_SHORT, MA_Z_CRC = 1, 2, 4, 8, 16
MA_X_BAD_RECORD = 1


class Bgzf(C.Structure):
    """ma_bgzf_t: compressed BGZF members and where each begins"""
    _fields_ = [("n_blocks", C.c_int64), ("cblob", C.c_void_p), ("cblob_bytes", C.c_uint64), ("blk_off", C.c_void_p),
                ("blk_len", C.c_void_p)]


class InflateOut(C.Structure):
    """ma_inflate_out_t: the capacity, then five arrays -- all required"""
    _fields_ = [("raw_cap", C.c_uint64)] + [(n, C.c_void_p) for n in ("raw", "blk_raw_off", "blk_state", "n_raw", "n_flagged")]


class RecordStreams(C.Structure):
    """ma_record_streams_t: inflated BAM bytes and the byte ranges whose records are wanted"""
    _fields_ = [("raw", C.c_void_p), ("raw_bytes", C.c_uint64), ("n_streams", C.c_int64), ("str_begin", C.c_void_p),
                ("str_end", C.c_void_p)]


class IndexOut(C.Structure):
    """ma_index_out_t: the capacity, then eight arrays -- all required"""
    _fields_ = [("rec_cap", C.c_uint64)] + [(n, C.c_void_p) for n in (
        "n_found", "str_rec_off", "str_state", "rec_off", "rec_len", "rec_ref", "rec_pos", "rec_span")]


BGZF_DTYPES = dict(cblob=np.uint8, blk_off=np.uint64, blk_len=np.uint32)
STREAMS_DTYPES = dict(raw=np.uint8, str_begin=np.uint64, str_end=np.uint64)


def inflate_out_spec(n_blocks, raw_cap):
    """arrays of ma_inflate_out_t (ma_inflate_blocks_batch)"""
    n = int(n_blocks)
    return dict(raw=(np.uint8, int(raw_cap)), blk_raw_off=(np.uint64, n + 1), blk_state=(np.uint8, n), n_raw=(np.uint64, 1),
                n_flagged=(np.uint64, 1))


def index_out_spec(n_streams, rec_cap):
    """arrays of ma_index_out_t (ma_index_records_batch)"""
    n, r = int(n_streams), int(rec_cap)
    return dict(n_found=(np.uint64, 1), str_rec_off=(np.uint64, n + 1), str_state=(np.uint8, n), rec_off=(np.uint64, r),
                rec_len=(np.uint32, r), rec_ref=(np.int32, r), rec_pos=(np.int32, r), rec_span=(np.uint32, r))


def make_bgzf_struct(arrays, n_blocks, cblob_bytes):
    """ma_bgzf_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller)"""
    s = fill_struct(Bgzf, arrays)
    s.n_blocks, s.cblob_bytes = int(n_blocks), int(cblob_bytes)
    return s


def make_inflate_out(arrays, raw_cap):
    s = fill_struct(InflateOut, arrays)
    s.raw_cap = int(raw_cap)
    return s


def make_streams_struct(arrays, n_streams, raw_bytes):
    """ma_record_streams_t over a dict of arrays (numpy, torch tensors or raw pointers; kept alive by the caller)"""
    s = fill_struct(RecordStreams, arrays)
    s.n_streams, s.raw_bytes = int(n_streams), int(raw_bytes)
    return s


def make_index_out(arrays, rec_cap):
    s = fill_struct(IndexOut, arrays)
    s.rec_cap = int(rec_cap)
    return s


def gate_out_spec(n):
    return dict(max_approx=(np.uint32, n), max_exact=(np.uint32, n))


def alloc_host(spec):
    return {k: np.zeros(sz, dtype=dt) for k, (dt, sz) in spec.items()}


def fill_struct(cls, arrays):
    """Build a ctypes struct whose pointer fields reference numpy arrays (kept alive by caller)."""
    s = cls()
    for name, _ in cls._fields_:
        a = arrays.get(name) if isinstance(arrays, dict) else None
        if a is None:
            continue
        if isinstance(a, np.ndarray):
            setattr(s, name, a.ctypes.data)
        else:  # torch tensor or raw int pointer
            setattr(s, name, a if isinstance(a, int) else a.data_ptr())
    return s


def make_batch_struct(arrs, n_windows, n_reads):
    b = fill_struct(Batch, arrs)
    b.n_windows = n_windows
    b.n_reads = n_reads
    return b


def _pack_nibbles(codes, read_off):
    """4-bit codes (one per element, absolute positions of read_off) -> the nibble array of include/microasm.h: read r
    starts at byte (read_off[r] + r) >> 1, high nibble first."""
    off = np.asarray(read_off, dtype=np.int64)
    nr = len(off) - 1
    total = int(off[-1]) if nr > 0 else 0
    out = np.zeros((total + nr + 1) // 2, dtype=np.uint8)
    if total == 0:
        return out
    lens = off[1:] - off[:-1]
    read_of = np.repeat(np.arange(nr, dtype=np.int64), lens)
    within = np.arange(total, dtype=np.int64) - off[read_of]
    start = (off[:-1] + np.arange(nr, dtype=np.int64)) >> 1
    byte = start[read_of] + (within >> 1)
    shift = np.where(within & 1, 0, 4).astype(np.uint8)
    np.bitwise_or.at(out, byte, (codes.astype(np.uint8) & 15) << shift)
    return out


def unpack_nibbles(packed, read_off):
    """the inverse of _pack_nibbles: one 4-bit code per element"""
    off = np.asarray(read_off, dtype=np.int64)
    nr = len(off) - 1
    total = int(off[-1]) if nr > 0 else 0
    if total == 0:
        return np.zeros(0, dtype=np.uint8)
    lens = off[1:] - off[:-1]
    read_of = np.repeat(np.arange(nr, dtype=np.int64), lens)
    within = np.arange(total, dtype=np.int64) - off[read_of]
    start = (off[:-1] + np.arange(nr, dtype=np.int64)) >> 1
    b = packed[start[read_of] + (within >> 1)]
    return np.where(within & 1, b & 15, b >> 4).astype(np.uint8)


def pack_reads(arrs, qual_bits=None):
    """The read bases and qualities of a batch (dict of BATCH_DTYPES arrays) as ma_packed_reads_t wants them.  Bases that are
    none of BAM's sixteen letters (lower case included) become N, as in a BAM file.  qual_bits=None: 4 when the batch holds
    at most 16 distinct Phred values, else 8; asking for 4 with more than 16 raises.  Returns (packed, twin): packed =
    dict(bases4, quals, qual_bits, qual_dict), twin = a copy of `arrs` whose read_bases / read_quals are what the device
    decodes -- the input of the equivalent plain call."""
    read_off = np.asarray(arrs["read_off"], dtype=np.uint64)
    total = int(read_off[-1]) if len(read_off) > 1 else 0
    bases = np.asarray(arrs["read_bases"], dtype=np.uint8)[:total]
    quals = np.asarray(arrs["read_quals"], dtype=np.uint8)[:total]
    code_of = np.full(256, 15, dtype=np.uint8)
    for i, ch in enumerate(BASE_CODES):
        code_of[ord(ch)] = i
    codes = code_of[bases]
    letters = np.frombuffer(BASE_CODES.encode(), dtype=np.uint8)
    distinct = np.unique(quals)
    if qual_bits is None:
        qual_bits = 4 if len(distinct) <= 16 else 8
    if qual_bits not in (4, 8):
        raise ValueError("qual_bits must be 4 or 8")
    qual_dict = np.zeros(16, dtype=np.uint8)
    if qual_bits == 4:
        if len(distinct) > 16:
            raise ValueError(f"{len(distinct)} distinct qualities do not fit 4 bits")
        qual_dict[:len(distinct)] = distinct
        packed_quals = _pack_nibbles(np.searchsorted(distinct, quals).astype(np.uint8), read_off)
    else:
        packed_quals = np.ascontiguousarray(arrs["read_quals"], dtype=np.uint8).copy()
    packed = dict(bases4=_pack_nibbles(codes, read_off), quals=packed_quals, qual_bits=qual_bits, qual_dict=qual_dict)
    twin = dict(arrs)
    twin["read_bases"] = np.ascontiguousarray(arrs["read_bases"], dtype=np.uint8).copy()
    twin["read_bases"][:total] = letters[codes]
    twin["read_quals"] = np.ascontiguousarray(arrs["read_quals"], dtype=np.uint8).copy()
    return packed, twin


def make_packed_struct(packed):
    """ma_packed_reads_t over pack_reads()'s dict (numpy arrays, torch tensors or raw device pointers; kept alive by the caller)"""
    def ptr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else (a if isinstance(a, int) else a.data_ptr())
    s = PackedReads()
    s.bases4 = ptr(packed["bases4"])
    s.quals = ptr(packed["quals"])
    s.qual_bits = int(packed["qual_bits"])
    for i, v in enumerate(np.asarray(packed["qual_dict"], dtype=np.uint8)[:16]):
        s.qual_dict[i] = int(v)
    return s


def packed_batch_arrays(arrs):
    """the batch arrays of a packed call: everything but the read bases and qualities (those must be NULL)"""
    return {k: v for k, v in arrs.items() if k not in ("read_bases", "read_quals")}
