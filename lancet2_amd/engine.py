"""Thin Python binding over the C-ABI (libmicroasm.so) -- plumbing only.

The compute lives in the HIP library.  There is NO CPU fallback: constructing an Engine without the
built library or without a HIP device raises.
"""
import ctypes as C
import os

import numpy as np

from . import capi


class EngineError(RuntimeError):
    pass


def load_library(path=None):
    path = path or capi.LIB_PATH
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(the engine has no CPU fallback)")
    lib = capi.load_cdll(path)
    lib.ma_last_error.restype = C.c_char_p
    lib.ma_create.argtypes = [C.POINTER(capi.Params), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.ma_destroy.argtypes = [C.c_void_p]
    lib.ma_last_error.argtypes = [C.c_void_p]
    lib.ma_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.ma_synchronize.argtypes = [C.c_void_p]
    lib.ma_timing_control.argtypes = [C.c_void_p, C.c_int]
    lib.ma_repeat_gate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ma_assemble_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ma_msa_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ma_genotype_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ma_process_batch.argtypes = [C.c_void_p] * 6
    lib.ma_genotype_stats_batch.argtypes = [C.c_void_p] * 6
    lib.ma_process_stats_batch.argtypes = [C.c_void_p] * 7
    lib.ma_prefetch_batch.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "ma_process_packed_batch"):  # (absent from a build of before the packed calls given as `path` for an A/B)
        lib.ma_process_packed_batch.argtypes = [C.c_void_p] * 8
        lib.ma_prefetch_packed_batch.argtypes = [C.c_void_p] * 3
    if hasattr(lib, "ma_process_meta_batch"):  # (likewise: a build of before the read-metadata calls)
        lib.ma_genotype_meta_batch.argtypes = [C.c_void_p] * 8
        lib.ma_process_meta_batch.argtypes = [C.c_void_p] * 10
        lib.ma_prefetch_meta_batch.argtypes = [C.c_void_p] * 4
    if hasattr(lib, "ma_process_cx_batch"):  # (likewise: a build of before the annotation became a stage of the chain)
        lib.ma_process_cx_batch.argtypes = capi.PROCESS_CX_ARGTYPES
    lib.ma_annotate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    lib.ma_last_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_int]
    lib.ma_last_stats.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    lib.ma_set_streams.argtypes = [C.c_void_p, C.c_int]
    if hasattr(lib, "ma_set_poa_retry"):  # (likewise: a build of before the POA retry passes)
        lib.ma_set_poa_retry.argtypes = capi.SET_POA_RETRY_ARGTYPES
        lib.ma_last_poa_retry.argtypes = capi.LAST_POA_RETRY_ARGTYPES
    if hasattr(lib, "ma_assemble_graph_batch"):  # (likewise: a build of before the graph export)
        lib.ma_assemble_graph_batch.argtypes = [C.c_void_p] * 4
        lib.ma_last_graph_export.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(lib, "ma_assemble_probe_batch"):  # (likewise: a build of before the probe call)
        lib.ma_assemble_probe_batch.argtypes = [C.c_void_p] * 5
    if hasattr(lib, "ma_msa_graph_batch"):  # (likewise: a build of before the POA export)
        lib.ma_msa_graph_batch.argtypes = [C.c_void_p] * 5
        lib.ma_last_poa_export.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_int]
    if hasattr(lib, "ma_flatten_records_batch"):  # (likewise: a build of before the record flattening)
        lib.ma_flatten_records_batch.argtypes = [C.c_void_p] * 3
    if hasattr(lib, "ma_select_records_batch"):  # (likewise: a build of before the record selection)
        lib.ma_select_records_batch.argtypes = [C.c_void_p] * 4
    if hasattr(lib, "ma_inflate_blocks_batch"):  # (likewise: a build of before the device inflate)
        lib.ma_inflate_blocks_batch.argtypes = [C.c_void_p] * 3
        lib.ma_index_records_batch.argtypes = [C.c_void_p] * 3
    return lib


class Engine:
    """Mirrors the per-thread VariantBuilder of the reference (core/variant_builder.h:26-125): one
    Engine per GPU/stream, reused across batches of windows."""

    def __init__(self, params=None, device=0, memspace=capi.MA_MEM_HOST, lib_path=None):
        self.lib = load_library(lib_path)
        self.p = params or capi.default_params()
        self.memspace = memspace
        h = C.c_void_p()
        rc = self.lib.ma_create(C.byref(self.p), device, memspace, C.byref(h))
        if rc != 0:
            raise EngineError(f"ma_create failed with {rc} (-2 = no HIP device; the engine has no CPU fallback)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.ma_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError(f"{what} failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")

    def set_stream(self, stream_ptr):
        self._check(self.lib.ma_set_stream(self.h, C.c_void_p(stream_ptr)), "ma_set_stream")

    def synchronize(self):
        self._check(self.lib.ma_synchronize(self.h), "ma_synchronize")

    def timing_control(self, mode):
        self._check(self.lib.ma_timing_control(self.h, mode), "ma_timing_control")

    def kernel_times(self, cap=8192):
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        n = self.lib.ma_last_kernel_times(self.h, names, ms, cap)
        return [(names[i].decode(), float(ms[i])) for i in range(max(n, 0))]

    def set_streams(self, n):
        """Number of concurrent window ranges ma_process_batch uses (0 = automatic)."""
        self._check(self.lib.ma_set_streams(self.h, n), "ma_set_streams")

    def set_poa_retry(self, on):
        """1: windows whose POA graph overflowed are re-run by a second pass with a larger graph (include/microasm.h:
        ma_set_poa_retry); 0 (the default): they stay MA_W_VAR_OVERFLOW."""
        self._check(self.lib.ma_set_poa_retry(self.h, int(on)), "ma_set_poa_retry")

    def last_poa_retry(self):
        """Counts of include/microasm.h:ma_last_poa_retry for the last call that ran the POA stage."""
        buf = (C.c_ulonglong * 4)()
        n = self.lib.ma_last_poa_retry(self.h, buf, 4)
        return {k: int(buf[i]) for i, k in enumerate(capi.POA_RETRY_KEYS) if i < n}

    def stats(self):
        """Work counters of include/microasm.h:ma_last_stats."""
        buf = (C.c_ulonglong * 20)()
        n = self.lib.ma_last_stats(self.h, buf, 20)
        keys = ("pairs", "dp_pairs", "windows", "window_attempts", "dp_w41", "dp_w65", "dp_w129", "dp_wide",
                "distinct_kmers", "nodes_after_lowcov", "slow_instances", "kmer_instances", "edge_queue", "count_queue",
                "aln_dp_cells", "poa_band_cells", "poa_band_fills", "poa_full_cells", "poa_alignments", "poa_direct_alignments")
        return {k: int(buf[i]) for i, k in enumerate(keys) if i < n}

    # ---- host-array convenience (MA_MEM_HOST): numpy in, numpy out ----
    def _alloc(self, spec):
        if self.memspace != capi.MA_MEM_HOST:
            raise EngineError("numpy convenience calls need MA_MEM_HOST")
        return capi.alloc_host(spec)

    def gate(self, arrs, n, nr):
        out = self._alloc(capi.gate_out_spec(n))
        b = capi.make_batch_struct(arrs, n, nr)
        o = capi.fill_struct(capi.GateOut, out)
        self._check(self.lib.ma_repeat_gate_batch(self.h, C.byref(b), C.byref(o)), "ma_repeat_gate_batch")
        return out

    def assemble(self, arrs, n, nr):
        out = self._alloc(capi.asm_out_spec(self.p, n))
        b = capi.make_batch_struct(arrs, n, nr)
        o = capi.fill_struct(capi.AsmOut, out)
        self._check(self.lib.ma_assemble_batch(self.h, C.byref(b), C.byref(o)), "ma_assemble_batch")
        return out

    def assemble_graph(self, arrs, n, nr, max_nodes=512, max_edges=2048, max_seq_bytes=32768):
        """ma_assemble_graph_batch: assemble() + the pruned graph of every reported component (capi.graph_out_spec; the caps
        are per window).  Returns (asm, graph); graph also carries the three caps under their names."""
        out = self._alloc(capi.asm_out_spec(self.p, n))
        gr = self._alloc(capi.graph_out_spec(self.p, n, max_nodes, max_edges, max_seq_bytes))
        b = capi.make_batch_struct(arrs, n, nr)
        self.assemble_graph_device(b, capi.fill_struct(capi.AsmOut, out), capi.make_graph_struct(gr, max_nodes, max_edges, max_seq_bytes))
        gr.update(max_nodes=int(max_nodes), max_edges=int(max_edges), max_seq_bytes=int(max_seq_bytes))
        return out, gr

    def assemble_graph_device(self, batch_struct, asm, graph):
        """ma_assemble_graph_batch on caller-made structs (either memory space); graph=None: a null pointer, the plain call"""
        self._check(self.lib.ma_assemble_graph_batch(self.h, C.byref(batch_struct), C.byref(asm),
                                                     C.byref(graph) if graph is not None else None), "ma_assemble_graph_batch")

    def last_graph_export(self):
        """Windows exported by the last assemble_graph(), per clean route (include/microasm.h: ma_last_graph_export).  A window
        flagged MA_G_* is not counted; one that a capacity retry pass assembled again counts once per pass that wrote its rows."""
        buf = (C.c_ulonglong * 4)()
        n = self.lib.ma_last_graph_export(self.h, buf, 4)
        if n < 0:
            raise EngineError(f"ma_last_graph_export failed ({n}): {self.lib.ma_last_error(self.h).decode()}")
        return {k: int(buf[i]) for i, k in enumerate(capi.GRAPH_EXPORT_KEYS) if i < n}

    def assemble_probes(self, arrs, n, nr, probes):
        """ma_assemble_probe_batch: assemble() + one row per probe (include/microasm.h: ma_probe_out_t).  `probes`: the dict
        of capi.pack_probes -- probe_win_off[n + 1], then pos, ref_len, alt_off, alt_len per probe and the ALT pool.  Returns
        (asm, probe_out); raises EngineError with .rc = the ma_error."""
        pr = {k: np.ascontiguousarray(probes[k], dtype=dt) for k, dt in capi.PROBE_DTYPES.items()}
        n_probes = int(pr["probe_win_off"][n])
        out = self._alloc(capi.asm_out_spec(self.p, n))
        spec = capi.probe_out_spec(self.p, n_probes)
        po = self._alloc(spec)
        # (an empty array has no address worth passing: every member is required to be non-NULL)
        held = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in list(pr.items()) + list(po.items())}
        b = capi.make_batch_struct(arrs, n, nr)
        self.assemble_probes_device(b, capi.fill_struct(capi.AsmOut, out), capi.fill_struct(capi.Probes, held),
                                    capi.fill_struct(capi.ProbeOut, held))
        return out, po

    def assemble_probes_device(self, batch_struct, asm, probes, probe_out):
        """ma_assemble_probe_batch on caller-made structs (either memory space); probes / probe_out None: a null pointer,
        the plain call"""
        ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
        rc = self.lib.ma_assemble_probe_batch(self.h, C.byref(batch_struct), C.byref(asm), ref(probes), ref(probe_out))
        if rc != 0:
            e = EngineError(f"ma_assemble_probe_batch failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def flatten_records(self, rec_arrays, n_windows, n_records, bases_cap=None, n_refs=0):
        """ma_flatten_records_batch: raw BAM records (`rec_arrays`: the capi.RECORDS_DTYPES arrays, ref_map only with n_refs > 0)
        -> dict of the capi.flat_out_spec arrays, cut to what was written (bases4, read_quals) + 'bases_cap'.  bases_cap None:
        two thirds of the record bytes, which no batch of good records exceeds.  Raises EngineError with .rc = the ma_error and
        .n_bases = the need the call reported."""
        rec = {k: np.ascontiguousarray(rec_arrays[k], dtype=dt) for k, dt in capi.RECORDS_DTYPES.items()
               if rec_arrays.get(k) is not None and (k != "ref_map" or n_refs > 0)}
        if bases_cap is None:
            bases_cap = int(rec["rec_len"][:n_records].astype(np.uint64).sum()) * 2 // 3
        out = self._alloc(capi.flat_out_spec(n_records, bases_cap))
        # (an empty array has no address worth passing: every member is required to be non-NULL)
        held = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in list(rec.items()) + list(out.items())}
        rs = capi.make_records_struct(held, n_windows, n_records, n_refs, blob_bytes=rec["blob"].size)
        rs.n_samples_in = rec["sample_rank"].size
        try:
            self.flatten_records_device(rs, capi.make_flat_struct(held, bases_cap))
        except EngineError as e:
            e.n_bases = int(held["n_bases"][0])
            e.arrays = out
            raise
        total = int(held["n_bases"][0])
        out["n_bases"] = held["n_bases"]
        out["bases4"] = out["bases4"][:(total + n_records + 1) // 2]
        out["read_quals"] = out["read_quals"][:total]
        out["bases_cap"] = int(bases_cap)
        return out

    def flatten_records_device(self, records_struct, flat_struct):
        """ma_flatten_records_batch on caller-made structs (either memory space)"""
        rc = self.lib.ma_flatten_records_batch(self.h, C.byref(records_struct), C.byref(flat_struct))
        if rc != 0:
            e = EngineError(f"ma_flatten_records_batch failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def select_records(self, rec_arrays, n_windows, n_records, win_len, max_sample_cov=1000.0, min_anchor_cov=5,
                       skip_active_region=False):
        """ma_select_records_batch: the candidates of every window (`rec_arrays`: blob, rec_off, rec_len, rec_win_off,
        rec_sample and 'n_samples_in' or sample_rank for the sample count) -> dict of the capi.select_out_spec arrays, the four
        sel_ arrays cut to n_selected.  Raises EngineError with .rc = the ma_error and .arrays = the arrays as the call left
        them."""
        rec = {k: np.ascontiguousarray(rec_arrays[k], dtype=capi.RECORDS_DTYPES[k]) for k in capi.SELECT_IN_KEYS}
        n_samples = int(rec_arrays["n_samples_in"] if "n_samples_in" in rec_arrays else len(rec_arrays["sample_rank"]))
        rec["win_len"] = np.ascontiguousarray(win_len, dtype=np.uint32)
        out = self._alloc(capi.select_out_spec(n_windows, n_records, n_samples))
        # (an empty array has no address worth passing: every member is required to be non-NULL)
        held = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in list(rec.items()) + list(out.items())}
        rs = capi.make_records_struct(dict(held, n_samples_in=n_samples), n_windows, n_records, blob_bytes=rec["blob"].size)
        sp = capi.make_select_params(held["win_len"], max_sample_cov, min_anchor_cov, skip_active_region)
        try:
            self.select_records_device(rs, sp, capi.fill_struct(capi.SelectOut, held))
        except EngineError as e:
            e.arrays = out
            raise
        out["n_selected"] = held["n_selected"]
        total = int(held["n_selected"][0])
        for k in ("sel_off", "sel_len", "sel_sample", "sel_src"):
            out[k] = out[k][:total]
        return out

    def select_records_device(self, records_struct, select_params, select_out):
        """ma_select_records_batch on caller-made structs (either memory space)"""
        rc = self.lib.ma_select_records_batch(self.h, C.byref(records_struct), C.byref(select_params), C.byref(select_out))
        if rc != 0:
            e = EngineError(f"ma_select_records_batch failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def inflate_blocks(self, cblob, blk_off, blk_len, raw_cap=None):
        """ma_inflate_blocks_batch: BGZF members of `cblob` -> dict of the capi.inflate_out_spec arrays, raw cut to n_raw.
        Without raw_cap the call is re-submitted once with the need it reported.  Raises EngineError with .rc = the
        ma_error and .arrays = the arrays as the call left them."""
        ins = dict(cblob=np.ascontiguousarray(cblob, dtype=np.uint8), blk_off=np.ascontiguousarray(blk_off, dtype=np.uint64),
                   blk_len=np.ascontiguousarray(blk_len, dtype=np.uint32))
        n = len(ins["blk_off"])
        cap = int(raw_cap) if raw_cap is not None else 4 * ins["cblob"].size
        while True:
            out = self._alloc(capi.inflate_out_spec(n, cap))
            # (an empty array has no address worth passing: every member is required to be non-NULL)
            held = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in list(ins.items()) + list(out.items())}
            try:
                self.inflate_blocks_device(capi.make_bgzf_struct(held, n, ins["cblob"].size), capi.make_inflate_out(held, cap))
            except EngineError as e:
                need = int(held["n_raw"][0])
                if raw_cap is None and e.rc == capi.MA_ERR_ARG and need > cap:
                    cap = need
                    continue
                e.arrays = dict(out, n_raw=held["n_raw"], n_flagged=held["n_flagged"])
                raise
            out["n_raw"], out["n_flagged"] = held["n_raw"], held["n_flagged"]
            out["raw"] = out["raw"][:int(held["n_raw"][0])]
            return out

    def inflate_blocks_device(self, bgzf_struct, inflate_out):
        """ma_inflate_blocks_batch on caller-made structs (either memory space)"""
        rc = self.lib.ma_inflate_blocks_batch(self.h, C.byref(bgzf_struct), C.byref(inflate_out))
        if rc != 0:
            e = EngineError(f"ma_inflate_blocks_batch failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def index_records(self, raw, str_begin, str_end, rec_cap=None):
        """ma_index_records_batch: the records of byte ranges of `raw` -> dict of the capi.index_out_spec arrays, the five
        rec_ arrays cut to n_found.  Without rec_cap the call is re-submitted once with the need it reported."""
        ins = dict(raw=np.ascontiguousarray(raw, dtype=np.uint8), str_begin=np.ascontiguousarray(str_begin, dtype=np.uint64),
                   str_end=np.ascontiguousarray(str_end, dtype=np.uint64))
        n = len(ins["str_begin"])
        cap = int(rec_cap) if rec_cap is not None else ins["raw"].size // 256 + 16
        while True:
            out = self._alloc(capi.index_out_spec(n, cap))
            held = {k: (v if v.size else np.zeros(1, v.dtype)) for k, v in list(ins.items()) + list(out.items())}
            try:
                self.index_records_device(capi.make_streams_struct(held, n, ins["raw"].size), capi.make_index_out(held, cap))
            except EngineError as e:
                need = int(held["n_found"][0])
                if rec_cap is None and e.rc == capi.MA_ERR_ARG and need > cap:
                    cap = need
                    continue
                e.arrays = dict(out, n_found=held["n_found"])
                raise
            out["n_found"] = held["n_found"]
            for k in ("rec_off", "rec_len", "rec_ref", "rec_pos", "rec_span"):
                out[k] = out[k][:int(held["n_found"][0])]
            return out

    def index_records_device(self, streams_struct, index_out):
        """ma_index_records_batch on caller-made structs (either memory space)"""
        rc = self.lib.ma_index_records_batch(self.h, C.byref(streams_struct), C.byref(index_out))
        if rc != 0:
            e = EngineError(f"ma_index_records_batch failed ({rc}): {self.lib.ma_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def msa(self, arrs, n, nr, asm):
        out = self._alloc(capi.var_out_spec(self.p, n))
        b = capi.make_batch_struct(arrs, n, nr)
        a = capi.fill_struct(capi.AsmOut, asm)
        o = capi.fill_struct(capi.VarOut, out)
        self._check(self.lib.ma_msa_batch(self.h, C.byref(b), C.byref(a), C.byref(o)), "ma_msa_batch")
        return out

    def msa_graph(self, arrs, n, nr, asm, max_pnodes=4096, max_pedges=8192, max_cols=4096):
        """ma_msa_graph_batch: msa() + the SPOA graph and the MSA rows of every component (capi.poa_out_spec; max_pnodes and
        max_pedges are per window, max_cols per component).  Returns (var, poa); poa also carries the three caps under their
        names.  `asm`'s win_status may gain MA_W_VAR_OVERFLOW, as in msa()."""
        out = self._alloc(capi.var_out_spec(self.p, n))
        px = self._alloc(capi.poa_out_spec(self.p, n, max_pnodes, max_pedges, max_cols))
        b = capi.make_batch_struct(arrs, n, nr)
        self.msa_graph_device(b, capi.fill_struct(capi.AsmOut, asm), capi.fill_struct(capi.VarOut, out),
                              capi.make_poa_struct(px, max_pnodes, max_pedges, max_cols))
        px.update(max_pnodes=int(max_pnodes), max_pedges=int(max_pedges), max_cols=int(max_cols))
        return out, px

    def msa_graph_device(self, batch_struct, asm, var, poa):
        """ma_msa_graph_batch on caller-made structs (either memory space); poa=None: a null pointer, the plain call"""
        self._check(self.lib.ma_msa_graph_batch(self.h, C.byref(batch_struct), C.byref(asm), C.byref(var),
                                                C.byref(poa) if poa is not None else None), "ma_msa_graph_batch")

    def last_poa_export(self):
        """Windows the last msa_graph() ran with the export, per kind of pass (include/microasm.h: ma_last_poa_export)"""
        buf = (C.c_ulonglong * 4)()
        n = self.lib.ma_last_poa_export(self.h, buf, 4)
        if n < 0:
            raise EngineError(f"ma_last_poa_export failed ({n})")
        return {k: int(buf[i]) for i, k in enumerate(capi.POA_EXPORT_KEYS) if i < n}

    def genotype(self, arrs, n, nr, asm, var, debug=True):
        out = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        b = capi.make_batch_struct(arrs, n, nr)
        a = capi.fill_struct(capi.AsmOut, asm)
        v = capi.fill_struct(capi.VarOut, var)
        o = capi.fill_struct(capi.GenoOut, out)
        self._check(self.lib.ma_genotype_batch(self.h, C.byref(b), C.byref(a), C.byref(v), C.byref(o)),
                    "ma_genotype_batch")
        return out

    def genotype_stats(self, arrs, n, nr, asm, var, debug=False, fields=None):
        """ma_genotype_stats_batch: genotype() + the read-level FORMAT statistics (capi.fmt_out_spec; `fields`: a subset of
        its arrays, default all).  Returns (geno, fmt)."""
        out = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        fmt = self._alloc({k: s for k, s in capi.fmt_out_spec(self.p, n).items() if fields is None or k in fields})
        b = capi.make_batch_struct(arrs, n, nr)
        a = capi.fill_struct(capi.AsmOut, asm)
        v = capi.fill_struct(capi.VarOut, var)
        o = capi.fill_struct(capi.GenoOut, out)
        f = capi.fill_struct(capi.FmtOut, fmt)
        self._check(self.lib.ma_genotype_stats_batch(self.h, C.byref(b), C.byref(a), C.byref(v), C.byref(o), C.byref(f)),
                    "ma_genotype_stats_batch")
        return out, fmt

    def _fmt_pair(self, n, fields, meta_fields):
        fmt = self._alloc({k: s for k, s in capi.fmt_out_spec(self.p, n).items() if fields is None or k in fields})
        fmeta = self._alloc({k: s for k, s in capi.fmt_meta_out_spec(self.p, n).items()
                             if meta_fields is None or k in meta_fields})
        return fmt, fmeta

    def genotype_meta(self, arrs, meta, n, nr, asm, var, debug=False, fields=None, meta_fields=None):
        """ma_genotype_meta_batch: genotype_stats() + the six statistics over the read metadata (`meta`: dict of the four
        capi.META_DTYPES arrays; `meta_fields`: a subset of capi.fmt_meta_out_spec, default all).  Returns (geno, fmt, fmeta)."""
        out = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        fmt, fmeta = self._fmt_pair(n, fields, meta_fields)
        b = capi.make_batch_struct(arrs, n, nr)
        m = capi.fill_struct(capi.ReadMeta, meta)
        self._check(self.lib.ma_genotype_meta_batch(self.h, C.byref(b), C.byref(m), C.byref(capi.fill_struct(capi.AsmOut, asm)),
                                                    C.byref(capi.fill_struct(capi.VarOut, var)),
                                                    C.byref(capi.fill_struct(capi.GenoOut, out)),
                                                    C.byref(capi.fill_struct(capi.FmtOut, fmt)),
                                                    C.byref(capi.fill_struct(capi.FmtMetaOut, fmeta))), "ma_genotype_meta_batch")
        return out, fmt, fmeta

    def process_meta(self, arrs, meta, n, nr, packed=None, debug=False, fields=None, meta_fields=None):
        """ma_process_meta_batch: process_stats() -- process_packed() with `packed` (capi.pack_reads) -- + the statistics over
        the read metadata.  Returns (gate, asm, var, geno, fmt, fmeta)."""
        g = self._alloc(capi.gate_out_spec(n))
        a = self._alloc(capi.asm_out_spec(self.p, n))
        v = self._alloc(capi.var_out_spec(self.p, n))
        q = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        f, fm = self._fmt_pair(n, fields, meta_fields)
        b = capi.make_batch_struct(capi.packed_batch_arrays(arrs) if packed is not None else arrs, n, nr)
        pk = capi.make_packed_struct(packed) if packed is not None else None
        m = capi.fill_struct(capi.ReadMeta, meta)
        self.process_meta_device(b, pk, m, capi.fill_struct(capi.GateOut, g), capi.fill_struct(capi.AsmOut, a),
                                 capi.fill_struct(capi.VarOut, v), capi.fill_struct(capi.GenoOut, q),
                                 capi.fill_struct(capi.FmtOut, f), capi.fill_struct(capi.FmtMetaOut, fm))
        return g, a, v, q, f, fm

    def process_cx(self, arrs, n, nr, meta=None, packed=None, gc_frac=0.41, debug=False, fields=None, meta_fields=None):
        """ma_process_cx_batch: process_meta() + the annotation of annotate() as a stage of the chain.  `meta` None: without the
        statistics over the read metadata (fmeta comes back empty).  fmt / fmeta are passed as NULL when they hold no array.
        Returns (gate, asm, var, geno, fmt, fmeta, cx)."""
        g = self._alloc(capi.gate_out_spec(n))
        a = self._alloc(capi.asm_out_spec(self.p, n))
        v = self._alloc(capi.var_out_spec(self.p, n))
        q = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        f, fm = self._fmt_pair(n, fields, meta_fields if meta is not None else ())
        cx = self._alloc(capi.cx_out_spec(self.p, n))
        b = capi.make_batch_struct(capi.packed_batch_arrays(arrs) if packed is not None else arrs, n, nr)
        pk = capi.make_packed_struct(packed) if packed is not None else None
        m = capi.fill_struct(capi.ReadMeta, meta) if meta is not None else None
        self.process_cx_device(b, pk, m, capi.fill_struct(capi.GateOut, g), capi.fill_struct(capi.AsmOut, a),
                               capi.fill_struct(capi.VarOut, v), capi.fill_struct(capi.GenoOut, q),
                               capi.fill_struct(capi.FmtOut, f) if f else None,
                               capi.fill_struct(capi.FmtMetaOut, fm) if fm else None, capi.fill_struct(capi.CxOut, cx), gc_frac)
        return g, a, v, q, f, fm, cx

    def annotate(self, arrs, n, nr, asm, var, gc_frac=0.41):
        """VariantAnnotator (core/variant_annotator.cpp:43-101): SEQ_CX + GRAPH_CX of every variant."""
        out = self._alloc(capi.cx_out_spec(self.p, n))
        b = capi.make_batch_struct(arrs, n, nr)
        a = capi.fill_struct(capi.AsmOut, asm)
        v = capi.fill_struct(capi.VarOut, var)
        o = capi.fill_struct(capi.CxOut, out)
        self._check(self.lib.ma_annotate_batch(self.h, C.byref(b), C.byref(a), C.byref(v), C.c_double(gc_frac),
                                               C.byref(o)), "ma_annotate_batch")
        return out

    def process(self, arrs, n, nr, debug=False):
        g = self._alloc(capi.gate_out_spec(n))
        a = self._alloc(capi.asm_out_spec(self.p, n))
        v = self._alloc(capi.var_out_spec(self.p, n))
        q = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        b = capi.make_batch_struct(arrs, n, nr)
        self._check(self.lib.ma_process_batch(self.h, C.byref(b), C.byref(capi.fill_struct(capi.GateOut, g)),
                                              C.byref(capi.fill_struct(capi.AsmOut, a)),
                                              C.byref(capi.fill_struct(capi.VarOut, v)),
                                              C.byref(capi.fill_struct(capi.GenoOut, q))), "ma_process_batch")
        return g, a, v, q

    def process_stats(self, arrs, n, nr, debug=False, fields=None):
        """ma_process_stats_batch: process() + the read-level FORMAT statistics.  Returns (gate, asm, var, geno, fmt)."""
        g = self._alloc(capi.gate_out_spec(n))
        a = self._alloc(capi.asm_out_spec(self.p, n))
        v = self._alloc(capi.var_out_spec(self.p, n))
        q = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        f = self._alloc({k: s for k, s in capi.fmt_out_spec(self.p, n).items() if fields is None or k in fields})
        b = capi.make_batch_struct(arrs, n, nr)
        self._check(self.lib.ma_process_stats_batch(self.h, C.byref(b), C.byref(capi.fill_struct(capi.GateOut, g)),
                                                    C.byref(capi.fill_struct(capi.AsmOut, a)),
                                                    C.byref(capi.fill_struct(capi.VarOut, v)),
                                                    C.byref(capi.fill_struct(capi.GenoOut, q)),
                                                    C.byref(capi.fill_struct(capi.FmtOut, f))), "ma_process_stats_batch")
        return g, a, v, q, f

    def process_packed(self, arrs, n, nr, packed, debug=False, fields=None):
        """ma_process_packed_batch: process_stats() on packed reads (capi.pack_reads; the read_bases / read_quals of `arrs`,
        if any, are not passed).  Returns (gate, asm, var, geno, fmt)."""
        g = self._alloc(capi.gate_out_spec(n))
        a = self._alloc(capi.asm_out_spec(self.p, n))
        v = self._alloc(capi.var_out_spec(self.p, n))
        q = self._alloc(capi.geno_out_spec(self.p, n, nr, debug))
        f = self._alloc({k: s for k, s in capi.fmt_out_spec(self.p, n).items() if fields is None or k in fields})
        b = capi.make_batch_struct(capi.packed_batch_arrays(arrs), n, nr)
        pk = capi.make_packed_struct(packed)
        self._check(self.lib.ma_process_packed_batch(self.h, C.byref(b), C.byref(pk), C.byref(capi.fill_struct(capi.GateOut, g)),
                                                     C.byref(capi.fill_struct(capi.AsmOut, a)),
                                                     C.byref(capi.fill_struct(capi.VarOut, v)),
                                                     C.byref(capi.fill_struct(capi.GenoOut, q)),
                                                     C.byref(capi.fill_struct(capi.FmtOut, f))), "ma_process_packed_batch")
        return g, a, v, q, f

    # ---- device-resident path (MA_MEM_DEVICE): dicts of torch tensors (or raw int pointers) ----
    def process_device(self, batch_struct, gate, asm, var, geno):
        self._check(self.lib.ma_process_batch(self.h, C.byref(batch_struct), C.byref(gate), C.byref(asm),
                                              C.byref(var), C.byref(geno)), "ma_process_batch")

    def process_stats_device(self, batch_struct, gate, asm, var, geno, fmt):
        self._check(self.lib.ma_process_stats_batch(self.h, C.byref(batch_struct), C.byref(gate), C.byref(asm),
                                                    C.byref(var), C.byref(geno), C.byref(fmt)), "ma_process_stats_batch")

    def prefetch(self, batch_struct):
        """MA_MEM_HOST: start uploading the batch that the next process_device() call will be given (ma_prefetch_batch)."""
        self._check(self.lib.ma_prefetch_batch(self.h, C.byref(batch_struct)), "ma_prefetch_batch")

    def process_packed_device(self, batch_struct, packed_struct, gate, asm, var, geno, fmt=None):
        """ma_process_packed_batch on caller-made structs (either memory space); fmt=None: without the statistics"""
        self._check(self.lib.ma_process_packed_batch(self.h, C.byref(batch_struct), C.byref(packed_struct), C.byref(gate),
                                                     C.byref(asm), C.byref(var), C.byref(geno),
                                                     C.byref(fmt) if fmt is not None else None), "ma_process_packed_batch")

    def prefetch_packed(self, batch_struct, packed_struct):
        """MA_MEM_HOST: ma_prefetch_packed_batch -- prefetch() for the batch the next process_packed_device() call brings"""
        self._check(self.lib.ma_prefetch_packed_batch(self.h, C.byref(batch_struct), C.byref(packed_struct)),
                    "ma_prefetch_packed_batch")

    def genotype_meta_device(self, batch_struct, meta_struct, asm, var, geno, fmt=None, fmeta=None):
        """ma_genotype_meta_batch on caller-made structs (either memory space); None: a null pointer"""
        ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
        self._check(self.lib.ma_genotype_meta_batch(self.h, C.byref(batch_struct), ref(meta_struct), C.byref(asm), C.byref(var),
                                                    C.byref(geno), ref(fmt), ref(fmeta)), "ma_genotype_meta_batch")

    def process_meta_device(self, batch_struct, packed_struct, meta_struct, gate, asm, var, geno, fmt=None, fmeta=None):
        """ma_process_meta_batch on caller-made structs (either memory space); packed_struct=None: an ASCII batch"""
        ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
        self._check(self.lib.ma_process_meta_batch(self.h, C.byref(batch_struct), ref(packed_struct), ref(meta_struct),
                                                   C.byref(gate), C.byref(asm), C.byref(var), C.byref(geno), ref(fmt), ref(fmeta)),
                    "ma_process_meta_batch")

    def process_cx_device(self, batch_struct, packed_struct, meta_struct, gate, asm, var, geno, fmt, fmeta, cx, gc_frac=0.41):
        """ma_process_cx_batch on caller-made structs (either memory space); None: a null pointer"""
        ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
        self._check(self.lib.ma_process_cx_batch(self.h, C.byref(batch_struct), ref(packed_struct), ref(meta_struct),
                                                 C.byref(gate), C.byref(asm), C.byref(var), C.byref(geno), ref(fmt), ref(fmeta),
                                                 C.c_double(gc_frac), ref(cx)), "ma_process_cx_batch")

    def prefetch_meta(self, batch_struct, packed_struct, meta_struct):
        """MA_MEM_HOST: ma_prefetch_meta_batch -- prefetch() for the batch the next process_meta_device() call brings; the
        arguments in the C call's order (packed_struct=None: an ASCII batch)"""
        self._check(self.lib.ma_prefetch_meta_batch(self.h, C.byref(batch_struct),
                                                    C.byref(packed_struct) if packed_struct is not None else None,
                                                    C.byref(meta_struct)), "ma_prefetch_meta_batch")

    def annotate_device(self, batch_struct, asm, var, cx, gc_frac=0.41):
        self._check(self.lib.ma_annotate_batch(self.h, C.byref(batch_struct), C.byref(asm), C.byref(var),
                                               C.c_double(gc_frac), C.byref(cx)), "ma_annotate_batch")
