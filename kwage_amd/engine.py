"""Python mirror of the C ABI objects (include/kwage_amd.h): Context, Group, Batch, search.

Names and argument meaning follow the reference's search path: a Group is what the
reference reads slice by slice from `.db` files (kwage.cpp:414-416), a Batch is the set of query
strings handed to search() (kwage.cpp:119,137), SearchResult carries what search() appends to
its result map (MatchResult: num_kmers_found, num_query_kmer; kwage.cpp:534).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .native import Params, check, lib

SEARCH_EARLY_EXIT = 1
SEARCH_TIMING = 2
SEARCH_TIMING_KMER = 4

TOPK_MAX = native.TOPK_MAX

HIT_DTYPE = np.dtype([("query", "<u4"), ("column", "<u4"), ("num_match", "<u4")])


class Context:
    """One GPU + one HIP stream (kwage_ctx)."""

    def __init__(self, device: int = 0):
        self._h = C.c_void_p()
        check(lib().kwage_init(device, C.byref(self._h)))
        self.device = device

    def close(self) -> None:
        if self._h:
            lib().kwage_shutdown(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def mem_info(self) -> Tuple[int, int]:
        f, t = C.c_uint64(), C.c_uint64()
        check(lib().kwage_mem_info(self._h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def fingerprint(self) -> dict:
        """Identity of the device (kwage_device_fingerprint): uuid, name, arch, cus, clocks, pci -- filed with every measurement."""
        buf = C.create_string_buffer(512)
        check(lib().kwage_device_fingerprint(self._h, buf, 512))
        out = {}
        for kv in buf.value.decode("latin-1").split(";"):
            k, _, v = kv.partition("=")
            out[k] = int(v) if (v.isdigit() and k not in ("uuid", "pci")) else v
        return out

    def sync(self) -> None:
        check(lib().kwage_sync(self._h))

    def set_tuning(self, name: str, value: int) -> None:
        """One kernel-selection knob of this context (kwage_ctx_set_tuning; tests and tuning tools)."""
        check(lib().kwage_ctx_set_tuning(self._h, name.encode(), int(value)))

    def get_tuning(self, name: str) -> int:
        v = C.c_int64()
        check(lib().kwage_ctx_get_tuning(self._h, name.encode(), C.byref(v)))
        return int(v.value)

    def scratch_nonzero(self) -> dict:
        """Non-zero words left in the exchange buffers of the persistent gather kernels (kwage_ctx_scratch_nonzero):
        all zero between searches, or a cut pair was not finished."""
        out = (C.c_uint64 * 5)()
        check(lib().kwage_ctx_scratch_nonzero(self._h, out))
        return dict(zip(("walk_or", "walk_done", "band_or", "band_state", "cwalk_arrived"), (int(x) for x in out)))

    def refine_stats(self) -> list:
        """Per search slot: places of the cluster / item / unit lists the last early-exit search took, and the unit list's
        capacity (kwage_ctx_refine_stats)."""
        out = (C.c_uint64 * 8)()
        check(lib().kwage_ctx_refine_stats(self._h, out))
        return [dict(zip(("clusters", "items", "units", "units_cap"), (int(x) for x in out[4 * k:4 * k + 4]))) for k in range(2)]

    def tuning(self, **knobs):
        """`with ctx.tuning(walk_waves=17, walk_min_rows=1): ...` -- the knobs are set inside the block and put back
        after it."""
        ctx = self

        class _Scope:
            def __enter__(self):
                self.old = {k: ctx.get_tuning(k) for k in knobs}
                for k, v in knobs.items():
                    ctx.set_tuning(k, v)
                return ctx

            def __exit__(self, *exc):
                for k, v in self.old.items():
                    ctx.set_tuning(k, v)
        return _Scope()


class Group:
    """HBM-resident bit matrix of all columns sharing (kmer_len, num_hash, log_2_filter_len, hash_func)."""

    def __init__(self, ctx: Context, kmer_len: int, num_hash: int, log_2_filter_len: int,
                 column_capacity: int, hash_func: int = 0):
        self.ctx = ctx
        self.params = Params(kmer_len, num_hash, log_2_filter_len, hash_func)
        self._h = C.c_void_p()
        self._nrows = 1 << log_2_filter_len          # rows an add_columns() image must hold
        self._real: List[Tuple[int, int]] = []       # (first column, columns) of everything added: the rest of the span is padding
        self._column_bits = None                     # column_bits(), once computed
        self._tail = None                            # the open tail a live insert left (the next insert's column), None while closed
        check(lib().kwage_group_create(ctx._h, C.byref(self.params), column_capacity, C.byref(self._h)))

    @classmethod
    def sparse(cls, ctx: Context, kmer_len: int, num_hash: int, log_2_filter_len: int, column_capacity: int,
               rows: np.ndarray, hash_func: int = 0) -> "Group":
        """A group holding only the listed slices (sorted distinct row indices) of every file added to it
        (kwage_group_create_sparse): for a few queries against a large database."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        g = cls.__new__(cls)
        g.ctx = ctx
        g.params = Params(kmer_len, num_hash, log_2_filter_len, hash_func)
        g._h = C.c_void_p()
        g._nrows = int(rows.size)                     # a sparse group's images hold the listed rows only
        g._real = []
        g._column_bits = None
        g._tail = None
        check(lib().kwage_group_create_sparse(ctx._h, C.byref(g.params), column_capacity, rows.ctypes.data, rows.size, C.byref(g._h)))
        return g

    def close(self) -> None:
        if self._h:
            lib().kwage_group_destroy(self._h)
            self._h = C.c_void_p()

    def add_columns(self, rows: np.ndarray, num_filter: int) -> int:
        """rows: uint8 [2^L (a sparse group: its listed rows), >= ceil(num_filter/8)] host image of a file's bit-slice block."""
        assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.strides[1] == 1
        # the library reads exactly this many rows of host_row_stride bytes from the pointer
        assert rows.shape[0] == self._nrows and rows.shape[1] >= (num_filter + 7) // 8, (rows.shape, self._nrows, num_filter)
        first = C.c_uint64()
        check(lib().kwage_group_add_columns(self._h, rows.ctypes.data, rows.strides[0], num_filter, C.byref(first)))
        self._real.append((first.value, num_filter))
        self._tail = None
        return first.value

    def add_db_file(self, path: str) -> Tuple[int, int]:
        first, nf = C.c_uint64(), C.c_uint32()
        check(lib().kwage_group_add_db_file(self._h, path.encode(), C.byref(first), C.byref(nf)))
        self._real.append((first.value, nf.value))
        self._tail = None
        return first.value, nf.value

    def add_db_files(self, paths: Sequence[str]) -> List[Tuple[int, int]]:
        """Several files at once (columns in the order given): raw files stream through one copy-engine pipeline."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        first, nf = (C.c_uint64 * n)(), (C.c_uint32 * n)()
        check(lib().kwage_group_add_db_files(self._h, arr, n, first, nf))
        self._real.extend((int(first[i]), int(nf[i])) for i in range(n))
        self._tail = None
        return [(int(first[i]), int(nf[i])) for i in range(n)]

    def add_random_columns(self, num_columns: int, seed: int, density_q8: int) -> int:
        first = C.c_uint64()
        check(lib().kwage_group_add_random_columns(self._h, num_columns, seed, density_q8, C.byref(first)))
        self._real.append((first.value, num_columns))
        self._tail = None
        return first.value

    def _inserted(self, first: int, n: int) -> int:
        self._real.append((first, n))
        self._tail = first + n
        self._column_bits = None                     # (a live group changes: column_bits() is computed afresh)
        return first

    def insert_filters(self, bits, flags: int = 0) -> int:
        """Live insert (kwage_group_insert_filters): n whole Bloom filters become n new columns, before or after
        finalize(); returns the first one's column.  bits: uint8 [n, max(1, 2^L / 8)], LSB first -- `.bloom` payloads,
        kwage_bloom_bits_from_batch's output.  A numpy array takes the host form (rows may lie further apart than a
        filter), a CUDA tensor the device form."""
        first = C.c_uint64()
        if isinstance(bits, np.ndarray):
            assert bits.dtype == np.uint8 and bits.ndim == 2 and bits.shape[1] >= max(1, self._nrows // 8), bits.shape
            assert bits.shape[0] <= 1 or bits.strides[1] == 1 and bits.strides[0] >= bits.shape[1], bits.strides
            if bits.shape[0] and bits.strides[1] != 1:
                bits = np.ascontiguousarray(bits)
            check(lib().kwage_group_insert_filters(self._h, bits.ctypes.data if bits.size else None, bits.strides[0], bits.shape[0],
                                                   flags, C.byref(first), None))
        else:
            import torch
            assert bits.is_cuda and bits.dtype == torch.uint8 and bits.dim() == 2 and (bits.shape[0] <= 1 or bits.stride(1) == 1), "insert_filters: a uint8 [n, bytes] CUDA tensor"
            assert bits.shape[1] >= max(1, self._nrows // 8), bits.shape
            check(lib().kwage_group_insert_filters_device(self._h, bits.data_ptr() if bits.numel() else None, bits.stride(0), bits.shape[0],
                                                          flags, C.byref(first), None))
        return self._inserted(first.value, bits.shape[0])

    def insert_bloom_files(self, paths: Sequence[str], flags: int = 0) -> int:
        """The live insert from `.bloom` files (kwage_group_insert_bloom_files), columns in the order given; returns the
        first one's column."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        first = C.c_uint64()
        check(lib().kwage_group_insert_bloom_files(self._h, arr, n, flags, C.byref(first), None))
        return self._inserted(first.value, n)

    def retire_columns(self, cols: Sequence[int]) -> None:
        """Withdraw columns (kwage_group_retire_columns): pad columns from here on; compact() gives their space back."""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        check(lib().kwage_group_retire_columns(self._h, cols.ctypes.data if cols.size else None, cols.size))
        gone = sorted(set(int(c) for c in cols.tolist()))
        real = []
        for first, nf in self._real:                 # cut the retired columns out of the blocks that held them
            at = first
            for c in [c for c in gone if first <= c < first + nf]:
                if c > at:
                    real.append((at, c - at))
                at = c + 1
            if first + nf > at:
                real.append((at, first + nf - at))
        self._real = real
        self._column_bits = None

    def compact(self, timing: bool = False) -> Tuple[np.ndarray, dict]:
        """Close the gaps that retired columns and alignment pads leave, in place (kwage_group_compact): the m valid
        columns become columns 0 .. m - 1 in their order, the span shrinks and the next insert continues at column m.
        Returns (new_column, stats): int64 [old column_span], a column's new number or -1 for a pad or retired column,
        and the call's stats."""
        span = self.column_span
        new = np.empty(max(span, 1), dtype=np.uint64)
        st = native.CompactStats()
        check(lib().kwage_group_compact(self._h, SEARCH_TIMING if timing else 0, new.ctypes.data_as(C.POINTER(C.c_uint64)), span, C.byref(st)))
        new = new[:span].view(np.int64)              # (KWAGE_NO_COLUMN is -1 as int64)
        self._real = [(0, int(st.columns))] if st.columns else []
        self._tail = int(st.columns)
        self._column_bits = None
        return new, {f: getattr(st, f) for f, _ in native.CompactStats._fields_}

    def fold(self, log_2_filter_len: int, timing: bool = False) -> Tuple["Group", dict]:
        """A new group whose Bloom filters are 2^log_2_filter_len bits long (kwage_group_fold): every row of it the OR of the
        rows of this group that fall on it, made on the device -- bit for bit the group built from the same samples' filters
        at the short length.  Columns keep their numbers; the new group is finalized if this one is, open otherwise; this
        group is not changed.  Returns (group, stats)."""
        h = C.c_void_p()
        st = native.FoldStats()
        check(lib().kwage_group_fold(self._h, log_2_filter_len, SEARCH_TIMING if timing else 0, C.byref(h), C.byref(st)))
        g = Group.__new__(Group)
        g.ctx = self.ctx
        g.params = Params(self.params.kmer_len, self.params.num_hash, log_2_filter_len, self.params.hash_func)
        g._h = h
        g._nrows = 1 << log_2_filter_len
        g._real = list(self._real)
        g._column_bits = None
        g._tail = self._tail
        return g, {f: getattr(st, f) for f, _ in native.FoldStats._fields_}

    def copy_columns_from(self, src: "Group", cols: Optional[Sequence[int]] = None, timing: bool = False) -> Tuple[int, dict]:
        """Columns of another resident group become new columns of this one, packed on the device
        (kwage_group_copy_columns): cols[i] of `src` becomes column first_column + i, placed as insert_filters() places its
        filters; cols=None takes every valid column of `src`, ascending.  This group is afterwards bit for bit what
        insert_filters(src.export_filters(cols)) would have made of it; `src` is not changed.  Returns (first_column, stats)."""
        first = C.c_uint64()
        st = native.CopyStats()
        if cols is None:
            ptr, n = None, 0
        else:
            cols = np.ascontiguousarray(cols, dtype=np.uint64)
            ptr, n = cols.ctypes.data_as(C.c_void_p), cols.size      # (an empty list is refused: the pointer is not NULL)
        check(lib().kwage_group_copy_columns(self._h, src._h, ptr, n, SEARCH_TIMING if timing else 0, C.byref(first), C.byref(st)))
        self._inserted(first.value, int(st.columns))
        return first.value, {f: getattr(st, f) for f, _ in native.CopyStats._fields_}

    def union_columns(self, sets: Sequence[Sequence[int]], src: Optional["Group"] = None, timing: bool = False) -> Tuple[int, dict]:
        """New columns of this group, each the row-wise OR of listed columns of `src` (this group where src is None), made on
        the device (kwage_group_union_columns): column first_column + j is the Bloom filter of the union of the samples in
        sets[j].  From another group the columns are placed as insert_filters() places its filters; within one group they
        start at the next 16-byte boundary of the row, also behind an open tail (the columns skipped are pad columns:
        batch many unions into one call).  `src`'s own columns are not changed.  Returns (first_column, stats)."""
        src = self if src is None else src
        sets = [np.ascontiguousarray(s, dtype=np.uint64).reshape(-1) for s in sets]
        offsets = np.zeros(len(sets) + 1, dtype=np.uint64)
        if sets:
            offsets[1:] = np.cumsum([s.size for s in sets], dtype=np.uint64)
        columns = np.concatenate(sets) if sets else np.zeros(0, dtype=np.uint64)
        columns = columns if columns.size else np.zeros(1, dtype=np.uint64)      # (an empty list is refused by the call: the pointer is not NULL)
        first = C.c_uint64()
        st = native.UnionStats()
        check(lib().kwage_group_union_columns(self._h, src._h, columns.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), len(sets),
                                              SEARCH_TIMING if timing else 0, C.byref(first), C.byref(st)))
        self._inserted(first.value, int(st.sets))
        return first.value, {f: getattr(st, f) for f, _ in native.UnionStats._fields_}

    def _overlap_lists(self, cols, other, other_cols):
        """The lists of an overlap call as the C ABI takes them: (a's pointer, n_a, b's handle, b's pointer, n_b, cells
        [rows, columns], what the pointers point to)."""
        if other is None and other_cols is not None:
            raise ValueError("column_overlaps: other_cols without other (the symmetric form takes cols on both sides)")
        keep = [None if x is None else np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (cols, other_cols)]
        ptr = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in keep]      # (an empty list is refused: the pointer is not NULL)
        n = [0 if x is None else int(x.size) for x in keep]
        n_a = self.column_span if cols is None else n[0]
        n_b = n_a if other is None else other.column_span if other_cols is None else n[1]
        return ptr[0], n[0], (other._h if other is not None else None), ptr[1], n[1], (n_a, n_b), keep

    def column_overlaps(self, cols: Optional[Sequence[int]] = None, other: Optional["Group"] = None, other_cols: Optional[Sequence[int]] = None,
                        out=None, timing: bool = False):
        """The overlap matrix (kwage_group_column_overlaps_device): cell (i, j) = the rows in which column cols[i] of this
        group and column other_cols[j] of `other` are both set, as an integer matrix product on the matrix cores.  A list
        of None means every column of the span (dead columns give zeros); other=None is the symmetric form, cols against
        itself, of which only the upper tiles are computed.  Returns (cells, stats): cells an int32 device tensor
        [len(cols), len(other_cols)] holding the uint32 counts -- `out` where given (its columns beyond the cells are
        left alone)."""
        import torch
        pa, na, hb, pb, nb, (rows, width), keep = self._overlap_lists(cols, other, other_cols)
        if out is None:
            out = torch.empty((rows, width), dtype=torch.int32, device="cuda:%d" % self.ctx.device)
        _device_tensor(out, "out", torch.int32, row_multiple=1)
        if out.dim() != 2 or out.shape[0] != rows or out.shape[1] < width:
            raise ValueError("out: shape [%d, >= %d] required, got %s" % (rows, width, tuple(out.shape)))
        row_elems = out.stride(0) if out.shape[0] > 1 else max(out.shape[1], width)
        st = native.OverlapStats()
        # (an empty matrix has no address: the call refuses a NULL pointer and writes nothing through this one)
        check(lib().kwage_group_column_overlaps_device(self._h, pa, na, hb, pb, nb, out.data_ptr() or 1, row_elems, SEARCH_TIMING if timing else 0, C.byref(st)))
        stats = {f: getattr(st, f) for f, _ in native.OverlapStats._fields_}
        stats["kernel"] = (lib().kwage_group_overlap_kernel() or b"").decode()
        return out, stats

    def column_overlaps_host(self, cols: Optional[Sequence[int]] = None, other: Optional["Group"] = None, other_cols: Optional[Sequence[int]] = None,
                             timing: bool = False):
        """column_overlaps() through the host form (kwage_group_column_overlaps): (uint32 numpy [len(cols), len(other_cols)],
        stats)."""
        pa, na, hb, pb, nb, (rows, width), keep = self._overlap_lists(cols, other, other_cols)
        out = np.zeros((rows, width), dtype=np.uint32)
        st = native.OverlapStats()
        check(lib().kwage_group_column_overlaps(self._h, pa, na, hb, pb, nb, out.ctypes.data if out.size else 1, max(width, 1), SEARCH_TIMING if timing else 0, C.byref(st)))
        stats = {f: getattr(st, f) for f, _ in native.OverlapStats._fields_}
        stats["kernel"] = (lib().kwage_group_overlap_kernel() or b"").decode()
        return out, stats

    _NEIGHBOR_METRICS = {"shared": 0, "jaccard": 1}           # KWAGE_NEIGHBORS_SHARED, KWAGE_NEIGHBORS_JACCARD
    _NEIGHBORS_SKIP_SELF = 0x100                              # KWAGE_NEIGHBORS_SKIP_SELF

    def _neighbor_call(self, k, cols, other, other_cols, metric, min_shared, skip_self, timing):
        if other is None and other_cols is not None:
            raise ValueError("column_neighbors: other_cols without other (cols is then the candidate list as well)")
        if metric not in self._NEIGHBOR_METRICS:
            raise ValueError("column_neighbors: metric must be 'jaccard' or 'shared', got %r" % (metric,))
        pa, na, hb, pb, nb, (rows, _), keep = self._overlap_lists(cols, other, other_cols)
        flags = (SEARCH_TIMING if timing else 0) | (self._NEIGHBORS_SKIP_SELF if skip_self else 0)
        return (pa, na, hb, pb, nb, int(k), self._NEIGHBOR_METRICS[metric], int(min_shared)), flags, rows, keep

    @staticmethod
    def _neighbor_stats(st):
        stats = {f: getattr(st, f) for f, _ in native.NeighborsStats._fields_}
        stats["kernel"] = (lib().kwage_group_neighbors_kernel() or b"").decode()
        return stats

    def column_neighbors(self, k: int, cols: Optional[Sequence[int]] = None, other: Optional["Group"] = None, other_cols: Optional[Sequence[int]] = None,
                         metric: str = "jaccard", min_shared: int = 0, skip_self: bool = False, timing: bool = False):
        """Nearest-neighbour lists (kwage_group_column_neighbors_device): for every column of `cols` its k best partners among
        `other_cols` of `other` (cols itself where other is None), by Jaccard index or by shared set bits, in the exact order
        (key descending, index ascending), chosen on the device from the overlap matrix's cells strip by strip.  Lists as
        column_overlaps() takes them.  Returns (records, counts, stats): int32 device tensors [n_a, k, 4] -- (index, shared,
        bits of the column, bits of the partner) as uint32, (0xFFFFFFFF, 0, 0, 0) behind counts[i] -- and [n_a]."""
        import torch
        args, flags, rows, keep = self._neighbor_call(k, cols, other, other_cols, metric, min_shared, skip_self, timing)
        dev = "cuda:%d" % self.ctx.device
        records = torch.empty((rows, max(int(k), 0), 4), dtype=torch.int32, device=dev)
        counts = torch.empty((rows,), dtype=torch.int32, device=dev)
        st = native.NeighborsStats()
        # (an empty result has no address: the call refuses a NULL pointer and writes nothing through this one)
        check(lib().kwage_group_column_neighbors_device(self._h, *args, records.data_ptr() or 1, counts.data_ptr() or 1, flags, C.byref(st)))
        return records, counts, self._neighbor_stats(st)

    def column_neighbors_host(self, k: int, cols: Optional[Sequence[int]] = None, other: Optional["Group"] = None, other_cols: Optional[Sequence[int]] = None,
                              metric: str = "jaccard", min_shared: int = 0, skip_self: bool = False, timing: bool = False):
        """column_neighbors() through the host form (kwage_group_column_neighbors): (uint32 numpy [n_a, k, 4], uint32 numpy
        [n_a], stats)."""
        args, flags, rows, keep = self._neighbor_call(k, cols, other, other_cols, metric, min_shared, skip_self, timing)
        records = np.zeros((rows, max(int(k), 0), 4), dtype=np.uint32)
        counts = np.zeros((rows,), dtype=np.uint32)
        st = native.NeighborsStats()
        check(lib().kwage_group_column_neighbors(self._h, *args, records.ctypes.data if records.size else 1, counts.ctypes.data if counts.size else 1, flags, C.byref(st)))
        return records, counts, self._neighbor_stats(st)

    @staticmethod
    def _save_columns(columns: Sequence[int], sources: Sequence):
        """The kwage_save_column array of save_db() and export_bloom_files(): (array, what its entries point to -- to be
        kept alive until the call returns)."""
        n = len(columns)
        assert len(sources) == n, (len(sources), n)
        cols = (native.SaveColumn * max(n, 1))()
        keep = []
        for i, (c, src) in enumerate(zip(columns, sources)):
            cols[i].column = int(c)
            if isinstance(src, dict):
                si = native.SampleInfo()
                for k, v in src.items():
                    if k in ("attribute_tags", "attribute_values"):
                        arr = (C.c_char_p * len(v))(*[s.encode("latin-1") for s in v])
                        keep.append(arr)
                        setattr(si, k, arr)
                    else:
                        setattr(si, k, v.encode("latin-1") if isinstance(v, str) else v)
                keep.append(si)
                cols[i].info = C.pointer(si)
            elif src is not None:
                cols[i].source_db = str(src[0]).encode()
                cols[i].source_column = int(src[1])
        return cols, keep

    def save_db(self, path: str, columns: Sequence[int], sources: Sequence, staging_bytes: int = 0) -> dict:
        """Write the listed columns, in list order, as one raw `.db` file (kwage_group_save_db): gathered and packed on the
        device, byte for byte what kwage_build_db writes from the same filters.  sources[i] says where column i's
        FilterInfo record comes from: (db_path, column) copies it from that file, a dict of kwage_sample_info fields
        (at least run_accession) serializes it.  Returns the call's stats."""
        n = len(columns)
        cols, keep = self._save_columns(columns, sources)      # (keep: alive until the call returns)
        st = native.SaveStats()
        check(lib().kwage_group_save_db(self._h, path.encode(), cols, n, staging_bytes, C.byref(st)))
        return {"db_bytes": st.db_bytes, "runs": st.runs, "chunks": st.chunks, "extract_kernel_ms": st.extract_kernel_ms}

    def export_filters(self, cols: Sequence[int], out=None, staging_bytes: int = 0, timing: bool = False):
        """Export (kwage_group_export_filters): the listed columns, in list order (any order, repeats allowed), handed back
        as whole Bloom filters -- uint8 [n, max(1, 2^L / 8)], LSB first: `.bloom` payloads, what insert_filters() and
        FilterSet.from_bits() read -- transposed on the device.  out=None returns a new numpy array; a numpy `out` takes
        the host form (rows may lie further apart than a filter), a CUDA uint8 tensor `out` the device form; exactly the
        filters' bytes of `out` are written.  Returns the array (with timing=True: (array, kernel ms))."""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        n, fb = int(cols.size), max(1, self._nrows // 8)
        ms = C.c_float(0)
        flags = SEARCH_TIMING if timing else 0
        cptr = cols.ctypes.data_as(C.POINTER(C.c_uint64)) if n else None
        if out is None:
            out = np.empty((n, fb), dtype=np.uint8)
        if isinstance(out, np.ndarray):
            assert out.dtype == np.uint8 and out.ndim == 2 and out.shape[0] == n and out.shape[1] >= fb, out.shape
            assert out.shape[0] <= 1 or out.strides[1] == 1 and out.strides[0] >= out.shape[1], out.strides
            assert out.flags.writeable and (out.shape[0] == 0 or out.strides[1] == 1), "export_filters: a writable uint8 [n, bytes] array"
            check(lib().kwage_group_export_filters(self._h, cptr, n, out.ctypes.data if out.size else None, out.strides[0], staging_bytes, flags, C.byref(ms)))
        else:
            import torch
            assert out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == n and (out.shape[1] <= 1 or out.stride(1) == 1), "export_filters: a uint8 [n, bytes] CUDA tensor"
            assert out.shape[1] >= fb, out.shape
            check(lib().kwage_group_export_filters_device(self._h, cptr, n, out.data_ptr() if out.numel() else None, out.stride(0), flags, C.byref(ms)))
        return (out, ms.value) if timing else out

    def export_bloom_files(self, cols: Sequence[int], sources: Sequence, paths: Sequence[str], staging_bytes: int = 0) -> None:
        """Write the listed columns as `.bloom` files (kwage_group_export_bloom_files), column cols[i] to paths[i]: what
        kwage_build_db, insert_bloom_files() and `kwage_dbtool append` read.  sources as in save_db().  All files appear
        together once all are complete; a failure leaves none."""
        n = len(cols)
        assert len(paths) == n, (len(paths), n)
        sc, keep = self._save_columns(cols, sources)      # (keep: alive until the call returns)
        arr = (C.c_char_p * max(n, 1))(*[None if p is None else str(p).encode() for p in paths])
        check(lib().kwage_group_export_bloom_files(self._h, sc, arr, n, staging_bytes, 0, None))

    def set_bits(self, rows: np.ndarray, columns: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        columns = np.ascontiguousarray(columns, dtype=np.uint64)
        assert rows.shape == columns.shape
        check(lib().kwage_group_set_bits(self._h, rows.ctypes.data, columns.ctypes.data, rows.size))
        self._column_bits = None                     # (planted bits change the counts: column_bits() is computed afresh)

    def read_rows(self, rows: Sequence[int]) -> np.ndarray:
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        out = np.empty((rows.size, self.row_bytes), dtype=np.uint8)
        check(lib().kwage_group_read_rows(self._h, rows.ctypes.data, rows.size, out.ctypes.data, out.strides[0] if rows.size else self.row_bytes))
        return out

    def finalize(self) -> None:
        check(lib().kwage_group_finalize(self._h))

    def real_columns(self) -> np.ndarray:
        """bool [column_span]: the columns that hold a sample (the rest pads files to their byte boundaries)."""
        real = np.zeros(self.column_span, dtype=bool)
        for first, nf in self._real:
            real[first:first + nf] = True
        return real

    def column_bits(self) -> np.ndarray:
        """kwage_group_column_bits(): the set-bit count of every column (uint32 [column_span], 0 on pad columns) -- the
        denominator of a Jaccard index.  Computed once per group and kept until a live insert, retire, compaction or
        set_bits changes the group."""
        if self._column_bits is None:
            out = np.zeros(self.column_span, dtype=np.uint32)
            check(lib().kwage_group_column_bits(self._h, out.ctypes.data if out.size else None))
            self._column_bits = out
        return self._column_bits

    @property
    def room(self) -> int:
        """Columns a live insert (or copy_columns_from) could still take: the row's capacity behind where it would land."""
        landing = self._tail if self._tail is not None else (self.row_bytes + 15) // 16 * 16 * 8
        return max(0, 8 * self.row_stride - landing)

    num_columns = property(lambda self: lib().kwage_group_num_columns(self._h))
    column_span = property(lambda self: lib().kwage_group_column_span(self._h))
    row_bytes = property(lambda self: lib().kwage_group_row_bytes(self._h))
    row_stride = property(lambda self: lib().kwage_group_row_stride(self._h))
    device_bytes = property(lambda self: lib().kwage_group_device_bytes(self._h))

    @property
    def placement(self) -> dict:
        """How the matrix's device block was chosen (kwage_group_placement): candidates compared and the gather probe's
        GB/s on the block kept / released."""
        n, kept, other, win = C.c_uint32(), C.c_double(), C.c_double(), C.c_double()
        check(lib().kwage_group_placement(self._h, C.byref(n), C.byref(kept), C.byref(other), C.byref(win)))
        return {"candidates": n.value, "kept_probe_gbps": round(kept.value, 1), "other_probe_gbps": round(other.value, 1),
                "kept_windowed_probe_gbps": round(win.value, 1)}

    def stream_read_gbps(self, nbytes: int, iters: int = 3) -> float:
        g = C.c_double()
        check(lib().kwage_stream_read_gbps(self._h, nbytes, iters, C.byref(g)))
        return g.value


class Batch:
    """Query strings resident in HBM (kwage_batch)."""

    def __init__(self, ctx: Context, seqs: Sequence[bytes | str]):
        bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
        concat = b"".join(bs)
        self.ctx = ctx
        self.n = len(bs)
        self._h = C.c_void_p()
        check(lib().kwage_batch_create(ctx._h, concat, offs.ctypes.data, self.n, C.byref(self._h)))

    def close(self) -> None:
        if self._h:
            lib().kwage_batch_destroy(self._h)
            self._h = C.c_void_p()


@dataclass
class SearchResult:
    hits: np.ndarray                 # HIT_DTYPE, sorted by (query, column)
    num_query_kmer: np.ndarray       # uint32 per query
    query_threshold: np.ndarray      # uint32 per query
    total_kmers: int
    bit_tests: int
    algorithmic_bytes: int
    kmer_kernel_ms: float
    search_kernel_ms: float
    search_kernel_launches: int
    search_kernel: str = ""

    def per_query(self) -> List[List[Tuple[int, int]]]:
        out: List[List[Tuple[int, int]]] = [[] for _ in range(len(self.num_query_kmer))]
        for q, c, m in self.hits.tolist():
            out[q].append((c, m))
        return out


ZERO_COPY_HITS = 1 << 20      # longer hit lists are handed to numpy in place (the library's pinned block) instead of copied


class _ResultOwner:
    """Keeps a kwage_result alive for as long as a numpy view of its hit array exists; frees it (the pinned block goes
    back to the context's pool) when the view is collected."""

    def __init__(self, res):
        self.res = res

    def __del__(self):
        try:
            lib().kwage_result_free(self.res)
        except Exception:
            pass


def _unpack_result(res) -> SearchResult:
    free_now = True
    try:
        r = res.contents
        n = r.n_hits
        if n > ZERO_COPY_HITS:
            # 100 M records are 1.2 GB: no second copy (and no page faults) on the Python side either
            raw = (C.c_char * (n * HIT_DTYPE.itemsize)).from_address(C.addressof(r.hits.contents))
            raw._owner = _ResultOwner(res)          # numpy keeps `raw` alive, `raw` keeps the result alive
            free_now = False
            hits = np.frombuffer(raw, dtype=HIT_DTYPE)
        else:
            hits = np.empty(n, dtype=HIT_DTYPE)
            if n:
                C.memmove(hits.ctypes.data, r.hits, n * HIT_DTYPE.itemsize)
        nq = r.n_queries
        nk = np.ctypeslib.as_array(r.num_query_kmer, shape=(nq,)).copy() if nq else np.zeros(0, np.uint32)
        qt = np.ctypeslib.as_array(r.query_threshold, shape=(nq,)).copy() if nq else np.zeros(0, np.uint32)
        return SearchResult(hits, nk, qt, r.total_kmers, r.bit_tests, r.algorithmic_bytes,
                            r.kmer_kernel_ms, r.search_kernel_ms, r.search_kernel_launches,
                            (r.search_kernel or b"").decode())
    finally:
        if free_now:
            lib().kwage_result_free(res)


def search(group: Group, batch: Batch, threshold: float, flags: int = 0) -> SearchResult:
    """kwage_search(): every query of the batch against every column of the group."""
    res = C.POINTER(native.Result)()
    check(lib().kwage_search(group._h, batch._h, C.c_float(threshold), flags, C.byref(res)))
    return _unpack_result(res)


def search_topk(group: Group, batch: Batch, k: int, threshold: float = 0.0, flags: int = 0) -> SearchResult:
    """kwage_search_topk(): for every query, the k best-scoring columns of the group -- score = num_match, eligible the
    columns with score >= the floor (unsigned)(threshold * n), ordered by (score descending, column ascending) and cut at
    k.  Hits come back ordered by (query, column) like every other result; query_threshold holds the floor."""
    res = C.POINTER(native.Result)()
    check(lib().kwage_search_topk(group._h, batch._h, min(max(int(k), 0), 0xFFFFFFFF), C.c_float(threshold), flags, C.byref(res)))
    return _unpack_result(res)


def _device_tensor(t, name: str, dtype, cols: int = 0, row_multiple: int = 0):
    """row_multiple > 0: a 2-D tensor whose rows are contiguous and lie a multiple of that many elements apart (a block of
    columns of a wider matrix) is accepted as well."""
    import torch
    strided_rows = (row_multiple > 0 and isinstance(t, torch.Tensor) and t.dim() == 2 and (t.shape[1] <= 1 or t.stride(1) == 1)
                    and (t.shape[0] <= 1 or (t.stride(0) >= t.shape[1] and t.stride(0) % row_multiple == 0)))
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.dtype != dtype or not (t.is_contiguous() or strided_rows):
        raise ValueError("%s: a contiguous %s tensor on a device is required" % (name, dtype))
    if cols and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError("%s: shape [n, %d] required, got %s" % (name, cols, tuple(t.shape)))
    # the engine runs on its own stream: what torch queued for these tensors must be done first
    torch.cuda.current_stream(t.device).synchronize()
    return t


def search_topk_device_append(group: Group, batch: Batch, k: int, hits, count, column_base: int = 0, threshold: float = 0.0,
                              reset: bool = True, flags: int = 0, num_query_kmer=None) -> int:
    """kwage_search_topk_device_append(): search_topk's records left on the device, `column_base` added to their columns,
    appended to `hits` (int32 [capacity, 3] device tensor of (query, column, num_match) rows) behind the count[0]
    records already there; `count` is an int64 [1] device tensor (zeroed first when `reset`).  Records beyond the
    capacity are counted, not stored.  Returns the running total."""
    import torch
    _device_tensor(hits, "hits", torch.int32, 3)
    _device_tensor(count, "count", torch.int64)
    nk = 0 if num_query_kmer is None else _device_tensor(num_query_kmer, "num_query_kmer", torch.int32).data_ptr()
    total = C.c_uint64()
    check(lib().kwage_search_topk_device_append(group._h, batch._h, min(max(int(k), 0), 0xFFFFFFFF), C.c_float(threshold), flags,
                                                hits.data_ptr() or None, hits.shape[0], count.data_ptr(), int(column_base),
                                                1 if reset else 0, nk or None, C.byref(total)))
    return int(total.value)


def merge_topk_device(ctx: Context, hits, n_queries: int, k: int, order=None):
    """kwage_topk_merge_device(): top-k lists concatenated in `hits` (int32 [n, 3] device tensor of (query, column,
    num_match) rows, any order) merged to each query's first k records under (num_match descending, order[column]
    ascending; the column itself without `order`, an int32 device tensor indexed by column).  Returns an int32
    [m, 3] device tensor ordered by (query, column)."""
    import torch
    _device_tensor(hits, "hits", torch.int32, 3)
    n = hits.shape[0]
    cap = min(n, int(n_queries) * max(int(k), 0))
    out = torch.empty((max(cap, 1), 3), dtype=torch.int32, device=hits.device)
    count = torch.empty(1, dtype=torch.int64, device=hits.device)
    optr, n_order = None, 0
    if order is not None:
        _device_tensor(order, "order", torch.int32)
        optr, n_order = order.data_ptr() or None, order.numel()
    check(lib().kwage_topk_merge_device(ctx._h, hits.data_ptr() if n else None, n, int(n_queries), min(max(int(k), 0), 0xFFFFFFFF),
                                        optr, n_order, out.data_ptr(), cap, count.data_ptr()))
    return out[:int(count.item())]


@dataclass
class ScoreResult:
    scores: object                   # uint32 [n, span] numpy array (search_scores) / the caller's device tensor (search_scores_device)
    num_query_kmer: object           # uint32 per query, or None (search_scores_device without the tensor)
    kernel: str                      # "score_tile_kernel<10,1>", "count_kernel<7,1>+score_combine_kernel<14>", "" if nothing ran
    kernel_ms: float                 # with SEARCH_TIMING, else 0


def search_scores(group: Group, batch: Batch, flags: int = 0) -> ScoreResult:
    """kwage_search_scores(): the num_match of every column of the group for every query, as a uint32 [n, column_span]
    matrix (pad columns and queries without k-mers: 0)."""
    n, span = batch.n, group.column_span
    scores = np.zeros((n, span), dtype=np.uint32)
    nk = np.zeros(max(n, 1), dtype=np.uint32)
    ms = C.c_float(0)
    check(lib().kwage_search_scores(group._h, batch._h, scores.ctypes.data if scores.size else None, span, nk.ctypes.data, flags, C.byref(ms)))
    return ScoreResult(scores, nk[:n], (lib().kwage_search_scores_kernel() or b"").decode(), float(ms.value))


def search_scores_device(group: Group, batch: Batch, out, num_query_kmer=None, flags: int = 0) -> ScoreResult:
    """kwage_search_scores_device(): the same matrix written into `out`, an int32 device tensor [n, >= column_span] with
    unit inner stride and rows a multiple of 4 elements apart (a block of columns of a wider matrix will do); columns of
    `out` at or beyond the group's span are left alone.  num_query_kmer: None or an int32 [n] device tensor."""
    import torch
    _device_tensor(out, "out", torch.int32, row_multiple=4)
    span = group.column_span
    if out.dim() != 2 or out.shape[0] != batch.n or out.shape[1] < span:
        raise ValueError("out: shape [%d, >= %d] required, got %s" % (batch.n, span, tuple(out.shape)))
    row_elems = out.stride(0) if out.shape[0] > 1 else span      # (a single row: the distance between rows addresses nothing)
    nk = 0
    if num_query_kmer is not None:
        if _device_tensor(num_query_kmer, "num_query_kmer", torch.int32).numel() < batch.n:
            raise ValueError("num_query_kmer: %d elements required" % batch.n)
        nk = num_query_kmer.data_ptr()
    ms = C.c_float(0)
    check(lib().kwage_search_scores_device(group._h, batch._h, out.data_ptr() or None, row_elems, nk or None, flags, C.byref(ms)))
    return ScoreResult(out, num_query_kmer, (lib().kwage_search_scores_kernel() or b"").decode(), float(ms.value))


@dataclass
class PresenceResult:
    bits: object                     # uint8 [n, row_bytes] numpy array (search_presence) / the caller's device tensor (search_presence_device)
    passing: object                  # uint32 per query: the set bits of its row; None (search_presence_device without the tensor)
    num_query_kmer: object           # uint32 per query, or None (search_presence_device without the tensor)
    kernel: str                      # "presence_tile_kernel<10,1>", "count_kernel<7,1>+presence_combine_kernel<14>", "presence_and_kernel", "" if nothing ran
    kernel_ms: float                 # with SEARCH_TIMING, else 0

    def unpack(self) -> np.ndarray:
        """bool [n, column span]: cell (q, c) = bit c of row q (host results)."""
        bits = np.ascontiguousarray(self.bits)
        return np.unpackbits(bits, axis=1, bitorder="little").astype(bool) if bits.size else np.zeros((bits.shape[0], bits.shape[1] * 8), dtype=bool)


def presence_row_bytes(group: Group) -> int:
    """The bytes of a row that a presence search writes: the group's row bytes rounded up to 16."""
    return (group.row_bytes + 15) // 16 * 16


def search_presence(group: Group, batch: Batch, threshold: float, flags: int = 0) -> PresenceResult:
    """kwage_search_presence(): one bit per (query, column) of the group, set where kwage_search at the same threshold
    reports a record, as a uint8 [n, row_bytes] matrix in the byte order of the group's rows (pad bits and queries
    without k-mers: 0)."""
    n, w = batch.n, presence_row_bytes(group)
    buf = np.zeros((n, w), dtype=np.uint8)
    passing = np.zeros(max(n, 1), dtype=np.uint32)
    nk = np.zeros(max(n, 1), dtype=np.uint32)
    ms = C.c_float(0)
    check(lib().kwage_search_presence(group._h, batch._h, C.c_float(threshold), buf.ctypes.data if buf.size else None, w, passing.ctypes.data,
                                      nk.ctypes.data, flags, C.byref(ms)))
    return PresenceResult(buf[:, :group.row_bytes], passing[:n], nk[:n], (lib().kwage_search_presence_kernel() or b"").decode(), float(ms.value))


def search_presence_device(group: Group, batch: Batch, threshold: float, out, passing=None, num_query_kmer=None, flags: int = 0) -> PresenceResult:
    """kwage_search_presence_device(): the same bitmap written into `out`, a uint8 device tensor [n, >= W] (W: the
    group's row bytes rounded up to 16) with unit inner stride, rows a multiple of 16 bytes apart and a 16-byte aligned
    first byte (a block of columns of a wider matrix will do); bytes of `out` at or beyond W are left alone.  passing,
    num_query_kmer: None or int32 [n] device tensors."""
    import torch
    _device_tensor(out, "out", torch.uint8, row_multiple=16)
    w = presence_row_bytes(group)
    if out.dim() != 2 or out.shape[0] != batch.n or out.shape[1] < w:
        raise ValueError("out: shape [%d, >= %d] required, got %s" % (batch.n, w, tuple(out.shape)))
    row_bytes = out.stride(0) if out.shape[0] > 1 else w         # (a single row: the distance between rows addresses nothing)
    ptrs = []
    for t, name in ((passing, "passing"), (num_query_kmer, "num_query_kmer")):
        if t is not None and _device_tensor(t, name, torch.int32).numel() < batch.n:
            raise ValueError("%s: %d elements required" % (name, batch.n))
        ptrs.append(t.data_ptr() if t is not None else 0)
    ms = C.c_float(0)
    check(lib().kwage_search_presence_device(group._h, batch._h, C.c_float(threshold), out.data_ptr() or None, row_bytes, ptrs[0] or None,
                                             ptrs[1] or None, flags, C.byref(ms)))
    return PresenceResult(out, passing, num_query_kmer, (lib().kwage_search_presence_kernel() or b"").decode(), float(ms.value))


class FilterSet:
    """Whole Bloom filters as the questions of a search (kwage_filterset): their set rows as ascending row lists on the
    device.  Belongs to its context; close() it before the context."""

    def __init__(self, ctx: Context, params: Params, handle):
        self.ctx, self.params, self._h = ctx, params, handle

    @classmethod
    def from_columns(cls, group: Group, cols: Sequence[int]) -> "FilterSet":
        """The filters of the given global columns of a finalized, non-sparse group (kwage_filterset_from_columns)."""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        h = C.c_void_p()
        check(lib().kwage_filterset_from_columns(group._h, cols.ctypes.data if cols.size else None, cols.size, C.byref(h)))
        p = group.params
        return cls(group.ctx, Params(p.kmer_len, p.num_hash, p.log_2_filter_len, p.hash_func), h)

    @classmethod
    def from_bits(cls, ctx: Context, kmer_len: int, num_hash: int, log_2_filter_len: int, bits: np.ndarray, hash_func: int = 0) -> "FilterSet":
        """bits: uint8 [n, max(1, 2^L / 8)] host bit vectors, LSB first -- `.bloom` payloads, kwage_bloom_bits_from_batch's
        output (kwage_filterset_from_bits)."""
        bits = np.asarray(bits)
        if bits.dtype != np.uint8 or bits.ndim != 2 or bits.shape[1] != max(1, (1 << log_2_filter_len) // 8):
            raise ValueError("bits: uint8 [n, %d] required, got %s %s" % (max(1, (1 << log_2_filter_len) // 8), bits.dtype, bits.shape))
        bits = np.ascontiguousarray(bits)
        p = Params(kmer_len, num_hash, log_2_filter_len, hash_func)
        h = C.c_void_p()
        check(lib().kwage_filterset_from_bits(ctx._h, C.byref(p), bits.ctypes.data if bits.size else None, bits.shape[1], bits.shape[0], C.byref(h)))
        return cls(ctx, p, h)

    def close(self) -> None:
        if self._h:
            lib().kwage_filterset_destroy(self._h)
            self._h = C.c_void_p()

    def __len__(self) -> int:
        return int(lib().kwage_filterset_num_filters(self._h))

    n = property(__len__)

    def bit_counts(self) -> np.ndarray:
        out = np.zeros(len(self), dtype=np.uint32)
        check(lib().kwage_filterset_bit_counts(self._h, out.ctypes.data if out.size else None))
        return out

    def rows(self, i: int) -> np.ndarray:
        """Diagnostic: the row list of filter i, copied back (kwage_filterset_read_rows)."""
        count = C.c_uint64()
        check(lib().kwage_filterset_read_rows(self._h, i, None, 0, C.byref(count)))
        out = np.zeros(count.value, dtype=np.uint32)
        check(lib().kwage_filterset_read_rows(self._h, i, out.ctypes.data if out.size else None, out.size, C.byref(count)))
        return out


def search_filter_scores(group: Group, fs: FilterSet, flags: int = 0) -> ScoreResult:
    """kwage_search_filter_scores(): uint32 [filters, column_span], cell (i, c) = rows set in both filter i and column c
    (pad columns: 0).  num_query_kmer holds the filters' set-bit counts."""
    n, span = len(fs), group.column_span
    scores = np.zeros((n, span), dtype=np.uint32)
    ms = C.c_float(0)
    check(lib().kwage_search_filter_scores(group._h, fs._h, scores.ctypes.data if scores.size else None, span, flags, C.byref(ms)))
    return ScoreResult(scores, fs.bit_counts(), (lib().kwage_search_filter_kernel() or b"").decode(), float(ms.value))


def search_filter_scores_device(group: Group, fs: FilterSet, out, flags: int = 0) -> ScoreResult:
    """kwage_search_filter_scores_device(): the same matrix written into `out`, an int32 device tensor
    [filters, >= column_span] laid out as search_scores_device wants it; columns at or beyond the span are left alone."""
    import torch
    _device_tensor(out, "out", torch.int32, row_multiple=4)
    n, span = len(fs), group.column_span
    if out.dim() != 2 or out.shape[0] != n or out.shape[1] < span:
        raise ValueError("out: shape [%d, >= %d] required, got %s" % (n, span, tuple(out.shape)))
    row_elems = out.stride(0) if out.shape[0] > 1 else span
    ms = C.c_float(0)
    check(lib().kwage_search_filter_scores_device(group._h, fs._h, out.data_ptr() or None, row_elems, flags, C.byref(ms)))
    return ScoreResult(out, None, (lib().kwage_search_filter_kernel() or b"").decode(), float(ms.value))


class PendingSearch:
    """A submitted search (kwage_search_submit); collect() waits for it and returns the result."""

    def __init__(self, handle):
        self._h = handle

    def collect(self) -> SearchResult:
        h, self._h = self._h, None
        if h is None:
            raise native.KwageError(-6, "search already collected")
        res = C.POINTER(native.Result)()
        check(lib().kwage_search_collect(h, C.byref(res)))
        return _unpack_result(res)


def submit(group: Group, batch: Batch, threshold: float, flags: int = 0) -> PendingSearch:
    """First half of a search: the device pipeline is enqueued, the call returns at once.  At most two
    searches may be pending per context."""
    h = C.c_void_p()
    check(lib().kwage_search_submit(group._h, batch._h, C.c_float(threshold), flags, C.byref(h)))
    return PendingSearch(h)


Group.search = lambda self, batch, threshold, flags=0: search(self, batch, threshold, flags)
Group.search_topk = lambda self, batch, k, threshold=0.0, flags=0: search_topk(self, batch, k, threshold, flags)
Group.submit = lambda self, batch, threshold, flags=0: submit(self, batch, threshold, flags)
Group.search_scores = lambda self, batch, flags=0: search_scores(self, batch, flags)
Group.search_presence = lambda self, batch, threshold, flags=0: search_presence(self, batch, threshold, flags)
Group.search_filter_scores = lambda self, fs, flags=0: search_filter_scores(self, fs, flags)


def hash_batch(ctx: Context, kmer_len: int, num_hash: int, log_2_filter_len: int, batch: Batch
               ) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """Device k-mer stage alone: per query (distinct canonical k-mers, row indices [n, num_hash])."""
    p = Params(kmer_len, num_hash, log_2_filter_len, 0)
    offs = np.zeros(batch.n + 1, dtype=np.uint64)
    nk = np.zeros(max(batch.n, 1), dtype=np.uint32)
    # first call sizes the outputs (offsets are host-side arithmetic)
    check(lib().kwage_hash_batch(ctx._h, C.byref(p), batch._h, offs.ctypes.data, nk.ctypes.data, None, None))
    total = int(offs[-1])
    kmers = np.zeros(max(total, 1), dtype=np.uint64)
    rows = np.zeros(max(total, 1) * num_hash, dtype=np.uint32)
    check(lib().kwage_hash_batch(ctx._h, C.byref(p), batch._h, offs.ctypes.data, nk.ctypes.data,
                                 kmers.ctypes.data, rows.ctypes.data))
    out_k, out_r = [], []
    for i in range(batch.n):
        o, n = int(offs[i]), int(nk[i])
        out_k.append(kmers[o:o + n].copy())
        out_r.append(rows[o * num_hash:(o + n) * num_hash].reshape(n, num_hash).copy())
    return out_k, out_r


class Database:
    """Several Groups searched as one database -- what a KWAGE database directory is: `.db` files with
    different (kmer_len, num_hash, log_2_filter_len) because maestro picks the Bloom parameters per
    sample size (bloom.cpp:10-68 optimal_bloom_param), the adaptive / COBS-style layout of BASELINE
    config C5.  Hits carry the group index; columns are local to the group."""

    def __init__(self, groups: Sequence[Group]):
        self.groups = list(groups)

    @property
    def num_columns(self) -> int:
        return sum(g.num_columns for g in self.groups)

    @property
    def device_bytes(self) -> int:
        return sum(g.device_bytes for g in self.groups)

    def search(self, batch: Batch, threshold: float, flags: int = 0) -> List[SearchResult]:
        # the k-mer stage is re-run per group: row indices depend on log_2_filter_len (kwage.cpp:411-412)
        return [search(g, batch, threshold, flags) for g in self.groups]

    def search_topk(self, batch: Batch, k: int, threshold: float = 0.0) -> List[List[Tuple[int, int, int]]]:
        """Per query, the k best columns of the whole database under (score descending, group order, column ascending):
        every group's top-k list appended to one device list at its own column base (groups in order, so the global
        column IS the tie order), merged on the device.  Returns per query [(group, column, num_match), ...] in
        selection order."""
        import torch
        dev = torch.device("cuda", self.groups[0].ctx.device) if self.groups else None
        bases, at = [], 0
        for g in self.groups:
            bases.append(at)
            at += g.column_span
        if at > 1 << 32:
            raise OverflowError("Database.search_topk: %d columns do not fit the 32-bit column field" % at)
        out: List[List[Tuple[int, int, int]]] = [[] for _ in range(batch.n)]
        if not self.groups or not batch.n:
            return out
        hits = torch.empty((len(self.groups) * batch.n * min(max(int(k), 1), TOPK_MAX), 3), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        for gi, (g, base) in enumerate(zip(self.groups, bases)):
            n = search_topk_device_append(g, batch, k, hits, count, base, threshold, reset=(gi == 0))
        merged = merge_topk_device(self.groups[0].ctx, hits[:n], batch.n, k).cpu().numpy().view(np.uint32)
        import bisect
        for q, c, m in merged.tolist():
            gi = bisect.bisect_right(bases, c) - 1
            out[q].append((gi, c - bases[gi], m))
        for lst in out:
            lst.sort(key=lambda h: (-h[2], h[0], h[1]))
        return out

    def search_scores(self, batch: Batch):
        """Every query's score for every column of the whole database: one int32 device tensor [n, sum of the groups'
        column spans] in a single allocation, each group's block at the column base Database.search_topk gives it
        (groups in order); pad columns hold 0."""
        import torch
        if not self.groups:
            raise ValueError("Database.search_scores: no groups")
        dev = torch.device("cuda", self.groups[0].ctx.device)
        bases, at = [], 0
        for g in self.groups:
            bases.append(at)
            at += g.column_span
        out = torch.empty((batch.n, at), dtype=torch.int32, device=dev)
        for g, base in zip(self.groups, bases):
            if batch.n and g.column_span:
                search_scores_device(g, batch, out[:, base:base + g.column_span])
        return out

    def search_presence(self, batch: Batch, threshold: float, flags: int = 0):
        """Which columns of the whole database hold each query at the threshold: (uint8 device tensor [n, sum of the
        groups' W], bit bases) in a single allocation, W a group's row bytes rounded up to 16.  Each group's block
        starts at a 16-byte aligned byte of the row (the column bases of the score and top-k forms are multiples of 8
        columns only, too little for the kernels' 16-byte stores), so this form numbers the columns itself: column c of
        group i is bit bases[i] + c of a row, byte (bases[i] + c) // 8, bit (bases[i] + c) % 8.  Pad bits hold 0."""
        import torch
        if not self.groups:
            raise ValueError("Database.search_presence: no groups")
        dev = torch.device("cuda", self.groups[0].ctx.device)
        bases, at = [], 0
        for g in self.groups:
            bases.append(at * 8)
            at += presence_row_bytes(g)
        out = torch.empty((batch.n, at), dtype=torch.uint8, device=dev)
        for g, base in zip(self.groups, bases):
            w = presence_row_bytes(g)
            if batch.n and w:
                search_presence_device(g, batch, threshold, out[:, base // 8:base // 8 + w], flags=flags)
        return out, bases

    def similar(self, fs: "FilterSet", k: int) -> List[List[Tuple[int, int, int, int, int, float]]]:
        """Per filter of the set, the k samples of the database most like it by Jaccard index: the filter search of every
        group side by side in one int32 device tensor (as search_scores lays it out), then, in float64,
        shared / (filter_bits + column_bits - shared) -- 0 where that union is empty -- and each filter's first k real
        columns under (Jaccard descending, global column ascending) by a stable sort.  Groups whose parameters differ
        from the set's are left out: their filters are not comparable.  Returns per filter
        [(group index, column, shared, filter_bits, column_bits, jaccard), ...] in that order."""
        import torch
        n = len(fs)
        out: List[List[Tuple[int, int, int, int, int, float]]] = [[] for _ in range(n)]
        key = lambda p: (p.kmer_len, p.num_hash, p.log_2_filter_len, p.hash_func)
        groups = [(gi, g) for gi, g in enumerate(self.groups) if key(g.params) == key(fs.params) and g.column_span]
        if not n or not groups or k <= 0:
            return out
        dev = torch.device("cuda", groups[0][1].ctx.device)
        bases, at = [], 0
        for _, g in groups:
            bases.append(at)
            at += g.column_span
        shared = torch.empty((n, at), dtype=torch.int32, device=dev)
        for (_, g), base in zip(groups, bases):
            search_filter_scores_device(g, fs, shared[:, base:base + g.column_span])
        col_bits = torch.from_numpy(np.concatenate([g.column_bits() for _, g in groups]).astype(np.int64)).to(dev)
        real = torch.from_numpy(np.concatenate([g.real_columns() for _, g in groups])).to(dev)
        f_bits = torch.from_numpy(fs.bit_counts().astype(np.int64)).to(dev)
        sh = shared.to(torch.int64)
        union = f_bits[:, None] + col_bits[None, :] - sh
        jac = torch.where(union > 0, sh.to(torch.float64) / union.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
        jac = torch.where(real[None, :], jac, torch.full((), -1.0, dtype=torch.float64, device=dev))      # pad columns: behind every sample
        # (torch.topk leaves the order of ties open; a stable sort keeps equal values in column order)
        order = torch.sort(jac, dim=1, descending=True, stable=True).indices[:, :min(int(k), at)]
        take = lambda t: torch.gather(t, 1, order).cpu().numpy()
        o, j, s_, r = order.cpu().numpy(), take(jac), take(sh), take(real[None, :].expand(n, at))
        cb, fb = col_bits.cpu().numpy(), f_bits.cpu().numpy()
        import bisect
        for i in range(n):
            for c, jv, sv, ok in zip(o[i].tolist(), j[i].tolist(), s_[i].tolist(), r[i].tolist()):
                if ok:
                    gpos = bisect.bisect_right(bases, c) - 1
                    out[i].append((groups[gpos][0], c - bases[gpos], int(sv), int(fb[i]), int(cb[c]), float(jv)))
        return out

    def close(self) -> None:
        for g in self.groups:
            g.close()


@dataclass
class DatabaseHit:
    query: int
    path: str            # `.db` file the sample lives in
    column: int          # column within that file
    accession: str       # FilterInfo::csv_string() (run accession)
    num_kmers_found: int
    num_query_kmer: int


class _LiveBlock(str):
    """The `path` of a block of live-inserted samples in FileDatabase._layout: the string "live", carrying the run
    accessions recorded for the block's columns (no file holds them)."""
    def __new__(cls, accessions):
        self = super().__new__(cls, "live")
        self.accessions = list(accessions)
        return self


class FileDatabase(Database):
    """A directory tree / list of `.db` (`.dbz`) files loaded the way the `kwage` CLI loads it: files
    grouped by (kmer_len, num_hash, log_2_filter_len, hash_func), each group one HBM matrix; hits are
    mapped back to (file, column) and carry the sample's run accession.  With headroom > 0 every group has room for
    that many more columns: add_sample() makes new samples searchable in the resident groups (live insert),
    retire_sample() withdraws one, compact() gives the withdrawn samples' columns back to add_sample(), reserve() makes
    room again once the headroom is used up (a wider group, the columns copied on the device), merge_groups() makes one
    group of those that share their parameters."""

    def __init__(self, ctx: Context, paths: Sequence[str], headroom: int = 0):
        import os
        files: List[str] = []
        todo = list(paths)
        while todo:                                   # breadth first, like FindFiles (file_util.h:30-125)
            p = todo.pop(0)
            if os.path.isdir(p):
                for name in os.listdir(p):
                    full = p + "/" + name
                    if os.path.isdir(full):
                        todo.append(full)
                    elif full.lower().endswith((".db", ".dbz")):
                        files.append(full)
            elif os.path.isfile(p):
                files.append(p)
            else:
                raise native.KwageError(-3, "FindFiles::next: Unable to stat entry " + p)
        by_param = {}
        for f in files:
            h = native.DbHeader()
            check(lib().kwage_db_read_header(f.encode(), C.byref(h)))
            by_param.setdefault((h.kmer_len, h.num_hash, h.log_2_filter_len, h.hash_func), []).append((f, h.num_filter))
        groups, self._layout, self._info = [], [], {}
        for (k, nh, lg, hf), members in sorted(by_param.items()):
            span = 0
            for _, nf in members:
                span = (span + 15) // 16 * 16 + (nf + 7) // 8
            # (live inserts start on the 16-byte boundary behind the files)
            g = Group(ctx, k, nh, lg, span * 8 if headroom <= 0 else (span + 15) // 16 * 16 * 8 + headroom, hf)
            firsts = [(first, nf, f, 0) for (first, nf), (f, _) in zip(g.add_db_files([f for f, _ in members]), members)]
            g.finalize()
            groups.append(g)
            self._layout.append(firsts)
        super().__init__(groups)
        self.ctx = ctx
        self.files = files
        self._retired = set()                         # (group index, column) of the FILE columns retire_sample() withdrew

    def _blocks(self):
        """(group index, first column, columns, path, first column within the file) of every piece of the layout in report
        order: the files in file order (a file that compact() cut around a retired column: its pieces in column order),
        then the live blocks group by group.  A layout entry is (first column, columns, path, first column within the file)."""
        where = {}
        for gi, layout in enumerate(self._layout):
            for first, nf, path, f0 in layout:
                if not isinstance(path, _LiveBlock):
                    where.setdefault(path, []).append((gi, first, nf, path, f0))
        out = [piece for f in self.files for piece in where.get(f, [])]
        out.extend((gi, first, nf, path, f0) for gi, layout in enumerate(self._layout) for first, nf, path, f0 in layout if isinstance(path, _LiveBlock))
        return out

    def _samples(self):
        """(group index, column in the group, path, column in the block) of every sample in report order."""
        return [(gi, first + c, path, f0 + c) for gi, first, nf, path, f0 in self._blocks() for c in range(nf) if (gi, first + c) not in self._retired]

    def add_sample(self, accession: str, seqs: Sequence[bytes | str], group: int = 0) -> Tuple[int, int]:
        """Make one new sample searchable at once: its Bloom filter is built on the device from `seqs` at the parameters of
        group `group` (kwage_bloom_bits_from_batch: the exact k-mer set), inserted into that group's resident matrix
        (Group.insert_filters) and recorded under `accession` in a live block of the group's layout, whose path is "live".
        Returns (group index, column).  The group needs room: FileDatabase(..., headroom=n)."""
        g = self.groups[group]
        bits = np.zeros((1, max(1, (1 << g.params.log_2_filter_len) // 8)), dtype=np.uint8)
        b = Batch(self.ctx, seqs)
        try:
            distinct = C.c_uint64()
            check(lib().kwage_bloom_bits_from_batch(self.ctx._h, C.byref(g.params), b._h, bits.ctypes.data, C.byref(distinct)))
        finally:
            b.close()
        col = g.insert_filters(bits)
        self._layout[group].append((col, 1, _LiveBlock([accession]), 0))
        return group, col

    def retire_sample(self, accession: str) -> Tuple[int, int]:
        """Withdraw the first sample (in report order) carrying the run accession: Group.retire_columns on its column.
        Returns (group index, column); KeyError when no sample carries it."""
        for gi, col, path, c in self._samples():
            if self._accession(path, c) == accession:
                break
        else:
            raise KeyError("no sample with run accession %s in the database" % accession)
        self.groups[gi].retire_columns([col])
        if isinstance(path, _LiveBlock) and len(path.accessions) == 1:
            self._layout[gi] = [e for e in self._layout[gi] if e[2] is not path]
        else:                                         # (a file's column, or one of a live block of several: union_samples())
            self._retired.add((gi, col))
        return gi, col

    def union_samples(self, unions: Sequence[Tuple[str, Sequence[str]]], retire: bool = False) -> List[Tuple[int, int]]:
        """New samples that are unions of samples of the resident database, made on the device (Group.union_columns): for
        every (new_accession, member_accessions) one new column, the OR of the members' columns -- the Bloom filter of all
        their reads together, recorded under new_accession.  A member is the first sample in report order carrying the
        accession (retire_sample()'s rule); all members of one union must lie in one group.  One device call per group, the
        new samples of a group recorded in ONE live block, which save(), export_samples(), the searches and
        similar_samples() see like add_sample()'s.  retire=True withdraws the members afterwards: the "merge".  A group
        needs room for its unions behind the next 16-byte boundary of its row -- up to 127 columns more than their number
        (FileDatabase(..., headroom=n), reserve()).  KeyError for an unknown accession, ValueError for a union across two
        groups, both before anything changes.  Returns [(group index, column)] in the order of `unions`."""
        first = {}
        for gi, col, path, c in self._samples():
            first.setdefault(self._accession(path, c), (gi, col))
        per_group = {}                                # group index -> [(place in `unions`, new accession, member columns)]
        for i, (new, members) in enumerate(unions):
            members = list(members)
            if not members:
                raise ValueError("union %s has no members" % new)
            for a in members:
                if a not in first:
                    raise KeyError("no sample with run accession %s in the database" % a)
            gi = first[members[0]][0]
            for a in members:
                if first[a][0] != gi:
                    pa, pb = self.groups[gi].params, self.groups[first[a][0]].params
                    raise ValueError("union %s: %s lies in group %d (kmer_len %d, num_hash %d, log_2_filter_len %d) and %s in group %d "
                                     "(kmer_len %d, num_hash %d, log_2_filter_len %d): fold() and merge_groups() first"
                                     % (new, members[0], gi, pa.kmer_len, pa.num_hash, pa.log_2_filter_len,
                                        a, first[a][0], pb.kmer_len, pb.num_hash, pb.log_2_filter_len))
            per_group.setdefault(gi, []).append((i, new, [first[a][1] for a in members]))
        for gi, todo in per_group.items():            # room, before anything changes
            g = self.groups[gi]
            landing = (g.row_bytes + 15) // 16 * 16 * 8
            if landing + len(todo) > 8 * g.row_stride:
                raise native.KwageError(-1, "union_samples: group %d has no room for %d columns behind column %d of a row of %d: reserve() first"
                                        % (gi, len(todo), landing, 8 * g.row_stride))
        out = [None] * len(unions)
        for gi, todo in per_group.items():
            col, _ = self.groups[gi].union_columns([cols for _, _, cols in todo])
            self._layout[gi].append((col, len(todo), _LiveBlock([new for _, new, _ in todo]), 0))
            for j, (i, _, _) in enumerate(todo):
                out[i] = (gi, col + j)
        if retire:
            gone = {}
            for gi, todo in per_group.items():
                for _, _, cols in todo:
                    gone.setdefault(gi, set()).update(cols)
            for gi, cols in gone.items():
                self.groups[gi].retire_columns(sorted(cols))
                single = {e[0] for e in self._layout[gi] if isinstance(e[2], _LiveBlock) and len(e[2].accessions) == 1 and e[0] in cols}
                self._layout[gi] = [e for e in self._layout[gi] if e[0] not in single or not isinstance(e[2], _LiveBlock)]
                self._retired.update((gi, c) for c in cols if c not in single)
        return out

    def compact(self) -> List[dict]:
        """Close the gaps that retired samples and the files' alignment pads leave, in every resident group
        (Group.compact): the freed columns are add_sample()'s again.  Columns are renumbered -- the layout follows, a file
        with a retired column in the middle becoming two pieces -- and every method answers as before, with the new
        numbers where it shows columns of a group.  Returns each group's stats."""
        stats = []
        for gi, g in enumerate(self.groups):
            new, st = g.compact()
            self._layout[gi] = self._renumbered(gi, new)
            self._retired = {(g2, c) for g2, c in self._retired if g2 != gi}
            stats.append(st)
        return stats

    def _renumbered(self, gi: int, new) -> list:
        """The layout of group gi after its columns moved: new[c] is column c's new number, negative for a column that is
        gone (a pad or retired column).  A block cut by a column that is gone becomes two pieces."""
        layout = []
        for first, nf, path, f0 in self._layout[gi]:
            kept = [c for c in range(nf) if new[first + c] >= 0]
            for i, c in enumerate(kept):
                if i and kept[i - 1] == c - 1:
                    at, n, p, f = layout[-1]
                    layout[-1] = (at, n + 1, p, f)
                else:
                    layout.append((int(new[first + c]), 1, path, f0 + c))
        return layout

    def _copied_into(self, dst: Group, gi: int) -> Tuple[list, dict]:
        """The valid columns of group gi copied, ascending, behind what `dst` holds (Group.copy_columns_from): (the
        group's layout under the new column numbers, the copy's stats -- {} for a group without columns)."""
        g = self.groups[gi]
        cols = np.flatnonzero(g.real_columns())
        new = np.full(max(g.column_span, 1), -1, dtype=np.int64)
        st = {}
        if cols.size:
            first, st = dst.copy_columns_from(g, cols)
            new[cols] = first + np.arange(cols.size)
        return self._renumbered(gi, new), st

    def reserve(self, headroom: int) -> List[dict]:
        """Room for `headroom` more add_sample() calls in every group, without a save and a reload: a group in which fewer
        columns fit behind where the next insert would land (Group.room) is replaced by a NEW group of its valid columns
        rounded up to 128, plus headroom, columns -- all valid columns copied on the device, ascending
        (Group.copy_columns_from), the new group finalized, the old one closed.  Columns are renumbered as compact()
        renumbers them, and every method answers as before.  An allocation that fails leaves the old group in place and
        raises.  Returns the stats of the copies made."""
        stats = []
        for gi, g in enumerate(self.groups):
            if g.room >= headroom:
                continue
            p = g.params
            wide = Group(self.ctx, p.kmer_len, p.num_hash, p.log_2_filter_len, (g.num_columns + 127) // 128 * 128 + headroom, p.hash_func)
            try:
                layout, st = self._copied_into(wide, gi)
                wide.finalize()
            except Exception:
                wide.close()
                raise
            self.groups[gi], self._layout[gi] = wide, layout
            self._retired = {(g2, c) for g2, c in self._retired if g2 != gi}
            g.close()
            stats.append(st)
        return stats

    def merge_groups(self) -> int:
        """Groups that share kmer_len, num_hash, log_2_filter_len and hash_func -- after fold(), or where the database was
        put together from several -- become ONE new group whose capacity is the sum of theirs: their valid columns copied
        on the device in group order (Group.copy_columns_from), the new group finalized, the old ones closed.  The new
        group takes the place of the first of them; layout entries and live blocks are re-attached under the new group
        index and column numbers (retired columns do not travel), so the report order of _blocks() stays: files in file
        order, then the live blocks group by group -- a merged group's at the place of its first member.  From then on a
        search runs once for them and save() writes one numbering.  Returns the number of groups removed."""
        members = {}
        for gi, g in enumerate(self.groups):
            p = g.params
            members.setdefault((p.kmer_len, p.num_hash, p.log_2_filter_len, p.hash_func), []).append(gi)
        merged = {}                                   # first member's index -> (new group, its layout)
        for (k, nh, lg, hf), gis in members.items():
            if len(gis) < 2:
                continue
            one = Group(self.ctx, k, nh, lg, sum(8 * self.groups[gi].row_stride for gi in gis), hf)
            try:
                layout = [e for gi in gis for e in self._copied_into(one, gi)[0]]
                one.finalize()
            except Exception:
                one.close()
                for g, _ in merged.values():
                    g.close()
                raise
            merged[gis[0]] = (one, layout)
        gone = {gi for gis in members.values() if len(gis) > 1 for gi in gis}
        groups, layouts, index = [], [], {}
        for gi, g in enumerate(self.groups):
            if gi in merged:
                g, layout = merged[gi]
            elif gi in gone:
                continue
            else:
                layout = self._layout[gi]
            index[gi] = len(groups)
            groups.append(g)
            layouts.append(layout)
        for gi in gone:
            self.groups[gi].close()
        removed = len(self.groups) - len(groups)
        self._retired = {(index[gi], c) for gi, c in self._retired if gi not in gone}
        self.groups, self._layout = groups, layouts
        return removed

    def fold(self, log_2_filter_len: int) -> List[dict]:
        """Shorten the Bloom filters of every resident group whose filters are longer than 2^log_2_filter_len bits to that
        length (Group.fold): the group is replaced by its fold and closed; groups at or below the length are left alone.
        Blocks, accessions, live and retired samples stay attached to the same column numbers, so save(), add_sample()
        (which hashes at the new length), retire_sample(), compact() and every search go on as on any database; two groups
        that now share their parameters stay two groups until merge_groups() makes them one.  Returns the stats of the
        groups folded."""
        stats = []
        for gi, g in enumerate(self.groups):
            if g.params.log_2_filter_len > log_2_filter_len:
                self.groups[gi], st = g.fold(log_2_filter_len)
                g.close()
                stats.append(st)
        return stats

    def save(self, out_dir: str, max_columns: int = 2048) -> List[str]:
        """Write the database as it stands -- live samples included, retired ones left out -- as `.db` files under out_dir
        (Group.save_db): group by group, every sample of _samples() in report order (file samples, then live samples), in
        files of at most max_columns columns (the reference's file width).  A file sample keeps the record of its own
        file; a live sample gets its recorded run accession and no other field.  FileDatabase(ctx, [out_dir]) afterwards
        answers as this database does.  Returns the files written."""
        import os
        assert max_columns >= 1
        os.makedirs(out_dir, exist_ok=True)
        written = []
        parts = {}                                    # (groups that share their parameters after fold(): the numbering goes on)
        for gi, g in enumerate(self.groups):
            mine = [(col, {"run_accession": path.accessions[c]} if isinstance(path, _LiveBlock) else (path, c))
                    for sgi, col, path, c in self._samples() if sgi == gi]
            p = g.params
            key = (p.kmer_len, p.log_2_filter_len, p.num_hash, p.hash_func)
            for at in range(0, len(mine), max_columns):
                piece = mine[at:at + max_columns]
                part = parts[key] = parts.get(key, -1) + 1
                out = os.path.join(out_dir, "k%d_L%d_h%d_f%d_%04d.db" % (key + (part,)))
                g.save_db(out, [c for c, _ in piece], [s for _, s in piece])
                written.append(out)
        return written

    def export_samples(self, accessions: Sequence[str], out_dir: str) -> List[str]:
        """Write samples of the resident database back as the `.bloom` files they were built from
        (Group.export_bloom_files): for each accession the first sample in report order carrying it, as
        <out_dir>/<accession>.bloom.  A file sample takes the record of its own file; a live sample gets its recorded run
        accession and no other field (save()'s rule).  KeyError, before anything is written, when no sample carries an
        accession.  Returns the files written."""
        import os
        first = {}
        for gi, col, path, c in self._samples():
            first.setdefault(self._accession(path, c), (gi, col, path, c))
        for a in accessions:
            if a not in first:
                raise KeyError("no sample with run accession %s in the database" % a)
        os.makedirs(out_dir, exist_ok=True)
        written = []
        for gi, g in enumerate(self.groups):
            mine = [(a,) + first[a][1:] for a in accessions if first[a][0] == gi]
            if mine:
                paths = [os.path.join(out_dir, a + ".bloom") for a, _, _, _ in mine]
                g.export_bloom_files([col for _, col, _, _ in mine],
                                     [{"run_accession": path.accessions[c]} if isinstance(path, _LiveBlock) else (path, c) for _, _, path, c in mine], paths)
                written.extend(paths)
        return written

    def _accession(self, path: str, column: int) -> str:
        if isinstance(path, _LiveBlock):
            return path.accessions[column]
        d = self._info.get(path)
        if d is None:
            d = C.c_void_p()
            check(lib().kwage_dbinfo_open(path.encode(), C.byref(d)))
            self._info[path] = d
        buf = C.create_string_buffer(64)
        check(lib().kwage_dbinfo_csv_string(d, column, buf, 64))
        return buf.value.decode()

    def search_sequences(self, seqs: Sequence[bytes | str], threshold: float = 1.0, flags: int = SEARCH_EARLY_EXIT) -> List[DatabaseHit]:
        """What `kwage -d ... <seqs>` reports, as records: sorted by query, then descending hits."""
        import bisect
        b = Batch(self.ctx, seqs)
        out: List[DatabaseHit] = []
        try:
            for g, layout in zip(self.groups, self._layout):
                r = search(g, b, threshold, flags)
                starts = [f[0] for f in layout]
                for q, c, m in r.hits.tolist():
                    i = bisect.bisect_right(starts, c) - 1
                    first, _, path, f0 = layout[i]
                    out.append(DatabaseHit(q, path, c - first + f0, self._accession(path, c - first + f0), m, int(r.num_query_kmer[q])))
        finally:
            b.close()
        out.sort(key=lambda h: (h.query, -h.num_kmers_found, h.path, h.column))
        return out

    def search_sequences_top(self, seqs: Sequence[bytes | str], k: int, threshold: float = 0.0) -> List[DatabaseHit]:
        """What `kwage_top -k <k> -t <threshold> -d ... <seqs>` reports, as records: per query the k best samples of the
        whole database under (score descending, file order, column ascending), listed by query, then descending hits.
        Each group's own top k is a superset of its share of the database's top k, so the merge is exact."""
        import bisect
        order = {f: i for i, f in enumerate(self.files)}
        b = Batch(self.ctx, seqs)
        per_query = {}
        try:
            for gi, (g, layout) in enumerate(zip(self.groups, self._layout)):
                r = search_topk(g, b, k, threshold)
                starts = [f[0] for f in layout]
                for q, c, m in r.hits.tolist():
                    i = bisect.bisect_right(starts, c) - 1
                    first, _, path, f0 = layout[i]
                    per_query.setdefault(q, []).append((m, path, c - first + f0, int(r.num_query_kmer[q]), gi, c))
        finally:
            b.close()
        out: List[DatabaseHit] = []
        for q in sorted(per_query):
            # (live samples rank behind every file, group by group in column order)
            best = sorted(per_query[q], key=lambda h: (-h[0], len(order) + h[4], h[5]) if isinstance(h[1], _LiveBlock) else (-h[0], order[h[1]], h[2]))[:k]
            out.extend(DatabaseHit(q, path, col, self._accession(path, col), m, nk) for m, path, col, nk, _, _ in best)
        return out

    def score_matrix(self, seqs: Sequence[bytes | str]) -> Tuple[np.ndarray, List[str]]:
        """What `kwage_scores -d ... <seqs>` prints, as (uint32 [n_queries, n_samples], run accessions): the real columns
        only, in file order then column order (live samples behind the files, retired ones left out)."""
        bases = np.cumsum([0] + [g.column_span for g in self.groups])
        samples = self._samples()
        cols = np.array([int(bases[gi]) + col for gi, col, _, _ in samples], dtype=np.int64)
        accessions = [self._accession(path, c) for _, _, path, c in samples]
        b = Batch(self.ctx, seqs)
        try:
            full = self.search_scores(b).cpu().numpy().view(np.uint32) if self.groups else np.zeros((b.n, 0), np.uint32)
        finally:
            b.close()
        return np.ascontiguousarray(full[:, cols]), accessions

    def presence_matrix(self, seqs: Sequence[bytes | str], threshold: float = 1.0) -> Tuple[np.ndarray, List[str]]:
        """What `kwage_presence -t <threshold> -d ... <seqs>` prints, as (bool [n_queries, n_samples], run accessions):
        the real columns only, in file order then column order (live samples behind the files, retired ones left out)."""
        b = Batch(self.ctx, seqs)
        try:
            if self.groups:
                packed, bases = self.search_presence(b, threshold)
                full = np.unpackbits(packed.cpu().numpy(), axis=1, bitorder="little").astype(bool)
            else:
                full, bases = np.zeros((b.n, 0), dtype=bool), []
        finally:
            b.close()
        samples = self._samples()
        cols = np.array([int(bases[gi]) + col for gi, col, _, _ in samples], dtype=np.int64)
        accessions = [self._accession(path, c) for _, _, path, c in samples]
        return np.ascontiguousarray(full[:, cols]), accessions

    def similar_samples(self, accessions: Sequence[str], k: int) -> List[Tuple[str, List[Tuple[str, str, int, int, int, int, float]]]]:
        """Per run accession, the k samples of the database most like it (Database.similar on its column): each accession
        is the first (file, column) carrying it, in file order; one not found raises KeyError.  Returns
        [(accession, [(sample accession, path, column in the file, shared, query_bits, sample_bits, jaccard), ...]), ...]."""
        import bisect
        found = {}
        for gi, col, path, c in self._samples():
            found.setdefault(self._accession(path, c), (gi, col))
        for a in accessions:
            if a not in found:
                raise KeyError("no sample with run accession %s in the database" % a)
        result = [None] * len(accessions)
        for gi in sorted({found[a][0] for a in accessions}):
            mine = [i for i, a in enumerate(accessions) if found[a][0] == gi]
            fs = FilterSet.from_columns(self.groups[gi], [found[accessions[i]][1] for i in mine])
            try:
                lists = self.similar(fs, k)
            finally:
                fs.close()
            for i, lst in zip(mine, lists):
                rec = []
                for g2, c, sh, fb, cb, jv in lst:
                    layout = self._layout[g2]
                    at = bisect.bisect_right([f[0] for f in layout], c) - 1
                    first, _, path, f0 = layout[at]
                    rec.append((self._accession(path, c - first + f0), path, c - first + f0, sh, fb, cb, jv))
                result[i] = (accessions[i], rec)
        return result

    def sample_overlaps(self, accessions: Optional[Sequence[str]] = None, jaccard: bool = False) -> Tuple[List[str], np.ndarray]:
        """The shared set bits of every pair of the chosen samples (all samples where accessions is None, in report order;
        an accession is the first (file, column) carrying it, one not found raises KeyError): Group.column_overlaps within
        a group in its symmetric form, between two groups of the same parameters in the a x b form, mirrored here.  Samples
        of groups whose parameters differ from the first chosen sample's are left out -- their filters are not comparable
        -- and named in a warning.  Returns (accessions, matrix): uint32 counts, the diagonal a sample's own bits; with
        jaccard=True float64 shared / (bits_i + bits_j - shared), 0 where that union is empty."""
        import warnings
        samples = [(gi, col, self._accession(path, c)) for gi, col, path, c in self._samples()]
        if accessions is not None:
            found = {}
            for gi, col, acc in samples:
                found.setdefault(acc, (gi, col, acc))
            for a in accessions:
                if a not in found:
                    raise KeyError("no sample with run accession %s in the database" % a)
            samples = [found[a] for a in accessions]
        if not samples:
            return [], np.zeros((0, 0), dtype=np.float64 if jaccard else np.uint32)
        key = lambda p: (p.kmer_len, p.num_hash, p.log_2_filter_len, p.hash_func)
        want = key(self.groups[samples[0][0]].params)
        left_out = [acc for gi, _, acc in samples if key(self.groups[gi].params) != want]
        if left_out:
            warnings.warn("sample_overlaps: %d samples of groups with other parameters are left out: %s" % (len(left_out), ", ".join(left_out)))
        samples = [s for s in samples if key(self.groups[s[0]].params) == want]
        n = len(samples)
        out = np.zeros((n, n), dtype=np.uint32)
        by_group = {}
        for i, (gi, col, _) in enumerate(samples):
            by_group.setdefault(gi, []).append(i)
        gis = sorted(by_group)
        for x, ga in enumerate(gis):
            ia = np.array(by_group[ga])
            ca = [samples[i][1] for i in ia]
            out[np.ix_(ia, ia)] = self.groups[ga].column_overlaps_host(ca)[0]
            for gb in gis[x + 1:]:
                ib = np.array(by_group[gb])
                cells = self.groups[ga].column_overlaps_host(ca, self.groups[gb], [samples[i][1] for i in ib])[0]
                out[np.ix_(ia, ib)] = cells
                out[np.ix_(ib, ia)] = cells.T
        names = [acc for _, _, acc in samples]
        if not jaccard:
            return names, out
        sh, bits = out.astype(np.int64), np.diag(out).astype(np.int64)
        union = bits[:, None] + bits[None, :] - sh
        return names, np.where(union > 0, sh.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)

    def sample_neighbors(self, k: int, accessions: Optional[Sequence[str]] = None, metric: str = "jaccard", min_shared: int = 0,
                         skip_self: bool = True) -> List[Tuple[str, List[Tuple[str, str, int, int, int, int, float]]]]:
        """Per chosen sample (every sample where accessions is None, in report order; an accession is the first (file,
        column) carrying it, one not found raises KeyError) its k most similar samples of the database, chosen on the
        device (Group.column_neighbors_host, one call per pair of query group and candidate group) and merged here under
        the same exact order -- the Jaccard index as a fraction, or the shared bits -- with ties in database order (group,
        then column).  The candidates are every sample of every resident group whose parameters equal the first chosen
        sample's; the samples of other groups are left out and named in a warning.  Returns
        [(accession, [(neighbour accession, path, column in the file, shared, query_bits, neighbour_bits, jaccard), ...]), ...]."""
        import warnings
        from fractions import Fraction
        every = [(gi, col, path, c, self._accession(path, c)) for gi, col, path, c in self._samples()]
        queries = every
        if accessions is not None:
            found = {}
            for s in every:
                found.setdefault(s[4], s)
            for a in accessions:
                if a not in found:
                    raise KeyError("no sample with run accession %s in the database" % a)
            queries = [found[a] for a in accessions]
        if not queries:
            return []
        key = lambda p: (p.kmer_len, p.num_hash, p.log_2_filter_len, p.hash_func)
        want = key(self.groups[queries[0][0]].params)
        left_out = [s[4] for s in every if key(self.groups[s[0]].params) != want]
        if left_out:
            warnings.warn("sample_neighbors: %d samples of groups with other parameters are left out: %s" % (len(left_out), ", ".join(left_out)))
        queries = [s for s in queries if key(self.groups[s[0]].params) == want]
        cands = {}                                            # group -> [(place in the database, sample)]
        for place, s in enumerate(every):
            if key(self.groups[s[0]].params) == want:
                cands.setdefault(s[0], []).append((place, s))
        by_group = {}
        for i, s in enumerate(queries):
            by_group.setdefault(s[0], []).append(i)
        lists = [[] for _ in queries]
        for ga in sorted(by_group):
            mine = by_group[ga]
            for gb in sorted(cands):
                rec, cnt, _ = self.groups[ga].column_neighbors_host(k, [queries[i][1] for i in mine], self.groups[gb], [s[1] for _, s in cands[gb]],
                                                                    metric=metric, min_shared=min_shared, skip_self=skip_self)
                for q, i in enumerate(mine):
                    for index, shared, bits_a, bits_b in rec[q, :cnt[q]].tolist():
                        union = bits_a + bits_b - shared
                        order = shared if metric == "shared" else (Fraction(shared, union) if union else Fraction(0))
                        place, s = cands[gb][index]
                        lists[i].append((-order, place, (s[4], s[2], s[3], shared, bits_a, bits_b, shared / union if union else 0.0)))
        return [(queries[i][4], [t[2] for t in sorted(lists[i], key=lambda t: t[:2])[:k]]) for i in range(len(queries))]

    def close(self) -> None:
        for d in self._info.values():
            lib().kwage_dbinfo_close(d)
        self._info = {}
        super().close()
