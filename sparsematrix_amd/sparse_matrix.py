"""Host-side mirror of the reference operator surface, over the C ABI.

``SparseMatrix`` follows ``sblas::SparseMatrix<uint8, uint8, float>``
(reference src/sparse/sparse-matrix.h:25-53) name for name: ``CopyForm``,
``CopyTo``, ``AddMatMat``, ``NumRows``, ``NumCols``, ``Destroy``,
``operator==`` (``__eq__``) and ``SelfTest``.  Host (numpy) operands go through
the synchronous, bit-exact ``sm_addmatmat_host``; device (torch, ``cuda``)
operands go through the asynchronous device entry points on the current
stream.  The device-level calls the benchmarks use are ``spmv`` / ``spmm``.

All arithmetic happens in the HIP kernels of libsparsematrix_amd.so.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import ALGOS, SM_NO_TRANS, SM_TRANS, SmInfo, check

SblasNoTrans = SM_NO_TRANS   # SBLAS_TRANSPOSE, sparse-matrix.h:20-23
SblasTrans = SM_TRANS


def _ptr(a) -> int:
    """Raw pointer of a numpy array or torch tensor (None -> 0)."""
    if a is None:
        return 0
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a.data_ptr())


def _is_device(a) -> bool:
    return a is not None and not isinstance(a, np.ndarray) and getattr(a, "is_cuda", False)


def _stream_of(t, stream) -> int:
    """`stream` as a raw handle; None: the current torch stream of t.device (a tensor's, or a
    SparseMatrix's device ordinal)."""
    if stream is not None:
        return int(stream) if isinstance(stream, int) else int(stream.cuda_stream)
    import torch
    return int(torch.cuda.current_stream(t.device).cuda_stream)


def _check_dev(t, min_elems: int, name: str) -> None:
    """Device operand guard: the C ABI takes raw pointers and cannot see sizes."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) torch tensor")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32")
    if t.numel() < min_elems:
        raise ValueError(f"{name} has {t.numel()} elements, needs at least {min_elems}")


def _check_dev_2d(t, rows: int, cols: int, name: str) -> None:
    _check_dev(t, 0, name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.shape[0] < rows \
            or t.shape[1] < cols:
        raise ValueError(f"{name} must be a row-major {rows} x {cols} (or larger) view")


def _sddmm_operand(t, rows: int, name: str):
    """(n_rhs, ld) of an sddmm operand: `rows` elements (1-D, unit stride: n_rhs = 1) or a
    row-major rows x n_rhs view (stride(1) == 1, stride(0) >= n_rhs)."""
    _check_dev(t, 0, name)
    if t.dim() == 1:
        if t.shape[0] != rows or (rows > 1 and t.stride(0) != 1):
            raise ValueError(f"{name} must be a unit-stride 1-D tensor of {rows} elements")
        return 1, 1
    if t.dim() != 2 or t.shape[0] != rows:
        raise ValueError(f"{name} must have {rows} elements (1-D) or {rows} rows (2-D), got {tuple(t.shape)}")
    n = int(t.shape[1])
    if n > 1 and t.stride(1) != 1:
        raise ValueError(f"{name} must be row-major (stride(1) == 1)")
    ld = int(t.stride(0)) if rows > 1 else n
    if ld < n:
        raise ValueError(f"{name} has stride(0) = {ld} < {n} columns")
    return n, ld


def _algo(algo) -> int:
    if isinstance(algo, int):
        return algo
    try:
        return ALGOS[algo]
    except KeyError:
        raise ValueError(f"algo must be one of {sorted(ALGOS)}") from None


class SparseMatrix:
    """sblas::SparseMatrix<uint8,uint8,float> on an MI355X (device-resident CSR of B = S^T)."""

    def __init__(self, density_matrix=None, rows: int = 0, cols: int = 0, stride: int = 0,
                 vals=None, val_table_size: int = 0, trans: int = SblasNoTrans,
                 device: int = 0):
        self._h = None
        self._t = None   # the cached transposed companion (T)
        self.device = device
        self._L = _lib.load()
        if density_matrix is not None:
            self.CopyForm(density_matrix, rows, cols, stride, vals, val_table_size, trans)

    # ---- lifetime ---------------------------------------------------------
    def Destroy(self) -> None:
        """sparse-matrix.cc:9-18.  Also releases the cached transposed companion (T)."""
        t, self._t = getattr(self, "_t", None), None
        if t is not None:
            t.Destroy()
        if self._h:
            self._L.sm_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.Destroy()
        except Exception:
            pass

    def _require(self):
        if not self._h:
            raise RuntimeError("SparseMatrix is empty (call CopyForm or from_csr first)")
        return self._h

    def _dims(self):
        """(n_rows, n_cols) of the held matrix, cached per handle: the per-call operand
        guards of spmv/spmm then cost no sm_get_info round trip."""
        h = self._require()
        if getattr(self, "_dims_h", None) != h:
            inf = self.info()
            self._dims_cache = (inf["n_rows"], inf["n_cols"])
            self._dims_h = h
        return self._dims_cache

    # ---- construction -----------------------------------------------------
    @classmethod
    def _created(cls, device: int, fn, head, opts: Optional[dict], tail, name: str) -> "SparseMatrix":
        """The shared end of the constructors that take sm_build_opts: a new matrix on `device`
        from the C function ``fn(*head, &opts, *tail, &handle)``, the status checked under `name`."""
        x = cls(device=device)
        o = _lib.build_opts(**(opts or {}))
        h = C.c_void_p()
        check(fn(*head, C.byref(o), *tail, C.byref(h)), name)
        x._h = h
        return x

    def CopyForm(self, density_matrix, rows: int, cols: int, stride: int, vals,
                 val_table_size: int, trans: int = SblasNoTrans) -> None:
        """sparse-matrix.cc:20-99: encode a rows x stride uint8 id matrix with a float table."""
        dm = np.ascontiguousarray(density_matrix, dtype=np.uint8).reshape(-1)
        if dm.size < rows * stride and rows * cols > 0 and val_table_size > 0:
            raise ValueError("density_matrix smaller than rows * stride")
        tb = np.zeros(max(int(val_table_size), 1), np.float32)
        if val_table_size:
            tb[:val_table_size] = np.asarray(vals, np.float32).reshape(-1)[:val_table_size]
        h = C.c_void_p()
        st = self._L.sm_create_from_dense_index(_ptr(dm), rows, cols, stride, _ptr(tb),
                                                val_table_size, int(trans), self.device,
                                                C.byref(h))
        check(st, "CopyForm")
        self.Destroy()
        self._h = h

    @classmethod
    def from_dense_index(cls, index, rows: int, cols: int, stride: int, vals,
                         val_table_size: int, trans: int = SblasNoTrans, device: int = 0,
                         stream=None) -> "SparseMatrix":
        """CopyForm from a uint8 id matrix (rows x stride): a torch cuda tensor is scanned
        on the device (sm_create_from_dense_index_device), anything else on the host."""
        self = cls(device=device)
        if not _is_device(index):
            self.CopyForm(index, rows, cols, stride, vals, val_table_size, trans)
            return self
        import torch
        assert index.dtype == torch.uint8
        dm = index.contiguous()
        if dm.numel() < rows * stride and rows * cols > 0 and val_table_size > 0:
            raise ValueError("index smaller than rows * stride")
        tb = np.zeros(max(int(val_table_size), 1), np.float32)
        if val_table_size:
            tb[:val_table_size] = np.asarray(vals, np.float32).reshape(-1)[:val_table_size]
        h = C.c_void_p()
        st = self._L.sm_create_from_dense_index_device(_ptr(dm), rows, cols, stride, _ptr(tb),
                                                       val_table_size, int(trans), device,
                                                       _stream_of(dm, stream), C.byref(h))
        check(st, "from_dense_index")
        self._h = h
        return self

    @classmethod
    def from_csr(cls, row_ptr, col_idx, val, n_cols: int, device: int = 0,
                 stream=None, opts: Optional[dict] = None) -> "SparseMatrix":
        """Additive CSR ingestion of B (n_rows x n_cols): numpy (host) or torch cuda tensors.

        `opts` (optional) forces the SpMV layout, e.g. ``{"layout": "exact"}`` or
        ``{"layout": "cband", "band_slabs": 1}`` -- the fields of sm_build_opts."""
        L = _lib.load()
        n_rows = int(row_ptr.shape[0]) - 1
        nnz = int(col_idx.shape[0])
        if _is_device(row_ptr):
            import torch
            assert row_ptr.dtype == torch.int32 and col_idx.dtype == torch.int32
            assert val.dtype == torch.float32
            rp, ci, va = row_ptr.contiguous(), col_idx.contiguous(), val.contiguous()
            return cls._created(device, L.sm_create_from_csr_device_ex,
                                (n_rows, n_cols, nnz, _ptr(rp), _ptr(ci), _ptr(va), device, _stream_of(rp, stream)),
                                opts, (), "from_csr")
        rp = np.ascontiguousarray(row_ptr, np.int32)
        ci = np.ascontiguousarray(col_idx, np.int32)
        va = np.ascontiguousarray(val, np.float32)
        return cls._created(device, L.sm_create_from_csr_ex, (n_rows, n_cols, nnz, _ptr(rp), _ptr(ci), _ptr(va), device),
                            opts, (), "from_csr")

    @classmethod
    def from_dense(cls, W, keep=None, per_row=None, threshold=None, opts: Optional[dict] = None,
                   stream=None) -> "SparseMatrix":
        """B from a dense float32 weight matrix on the device, selected and compacted there
        (sm_create_from_dense_device): exactly one of `keep` (the number of elements of greatest
        |value| of the whole matrix), `per_row` (of every row) and `threshold` (keep |value| >=
        threshold; the smallest subnormal keeps exactly the non-zeros, 0 keeps every element).  The
        rule is prune_mask's, on the full matrix in which every element of `W` is a stored term:
        ties go to the lower (row, column), a NaN is kept first.  The result is the matrix from_csr
        builds from the kept terms with the same `opts` (``{"updatable": 1}`` for fine-tuning).
        `W` is a 2-D float32 CUDA (HIP) tensor with ``stride(1) == 1``; ``stride(0)`` may exceed
        the row width, so padded and row-sliced views are read in place -- the padding is never
        read and `W` never written.  Nothing is copied silently: any other layout raises.
        Synchronises `stream` (None: the current torch stream)."""
        mode, count, thr = cls._prune_args(keep, per_row, threshold)
        if isinstance(W, np.ndarray) or not hasattr(W, "is_cuda"):
            raise TypeError("from_dense takes a torch tensor on the device; for host data build the CSR "
                            "(e.g. scipy.sparse.csr_matrix) and use from_csr")
        import torch
        if not W.is_cuda:
            raise TypeError("W is a host tensor: move it with W.cuda(), or build the CSR and use from_csr")
        if W.dtype != torch.float32:
            raise TypeError(f"W must be float32, got {W.dtype}: convert with W.float()")
        if W.dim() != 2:
            raise ValueError(f"W must be 2-D (n_rows x n_cols), got {W.dim()}-D: use W.reshape(n_rows, -1)")
        n_rows, n_cols = int(W.shape[0]), int(W.shape[1])
        if W.numel() and n_cols > 1 and W.stride(1) != 1:
            raise ValueError("W must be row-major (stride(1) == 1): use W.contiguous() (a transposed view "
                             "would be read as its transpose's memory)")
        ld = int(W.stride(0)) if n_rows > 1 and W.numel() else n_cols   # an empty tensor's strides say nothing
        if ld < n_cols:
            raise ValueError(f"W has stride(0) = {ld} < {n_cols} columns (an expanded view?): use W.contiguous()")
        return cls._created(W.device.index, _lib.load().sm_create_from_dense_device,
                            (_ptr(W) if W.numel() else 0, n_rows, n_cols, ld, mode, count, thr, W.device.index,
                             _stream_of(W, stream)), opts, (), "from_dense")

    @classmethod
    def from_csr_ids(cls, row_ptr, col_idx, ids, table, n_cols: int, device: int = 0,
                     opts: Optional[dict] = None) -> "SparseMatrix":
        """A table matrix (sm_create_from_csr_ids): the terms of B (n_rows x n_cols) as
        (row, col, id) plus one table of T <= 255 float32 values; term e stores table[ids[e]].
        Host (numpy) arrays; `ids`: nnz uint8 in CSR order, each < T.  Without options the matrix
        is what from_csr builds from ``table[ids]``; it also remembers ids and table, so
        sddmm_table applies.  ``opts={"table_updatable": 1}`` builds every layout in its codebook
        form from the given ids and table, so set_table / axpy_table replace the table in place.
        Torch device tensors (all four) go to from_csr_ids_device on the current torch stream."""
        if any(_is_device(a) for a in (row_ptr, col_idx, ids, table)):
            return cls.from_csr_ids_device(row_ptr, col_idx, ids, table, n_cols, device=device, opts=opts)
        rp = np.ascontiguousarray(row_ptr, np.int32)
        ci = np.ascontiguousarray(col_idx, np.int32)
        idv = np.ascontiguousarray(ids, np.uint8).reshape(-1)
        tb = np.ascontiguousarray(table, np.float32).reshape(-1)
        if idv.size != ci.size:
            raise ValueError(f"ids has {idv.size} elements, col_idx {ci.size}")
        if tb.size > 255 or (ci.size > 0 and tb.size < 1):
            raise ValueError(f"table must hold 1..255 values, got {tb.size}")
        return cls._created(device, _lib.load().sm_create_from_csr_ids,
                            (int(rp.shape[0]) - 1, n_cols, int(ci.size), _ptr(rp), _ptr(ci), _ptr(idv), _ptr(tb),
                             int(tb.size), device), opts, (), "from_csr_ids")

    @classmethod
    def from_csr_ids_device(cls, row_ptr, col_idx, ids, table, n_cols: int, device: int = 0,
                            opts: Optional[dict] = None, stream=None) -> "SparseMatrix":
        """from_csr_ids from torch tensors on `device` (sm_create_from_csr_ids_device): int32
        `row_ptr` / `col_idx`, uint8 `ids` (nnz, each < T), float32 `table` (T <= 255).  The result
        is the matrix from_csr_ids builds from the same arrays on the host, bit for bit; no array
        goes to the host unless ``opts={"table_updatable": 1}`` (then the ids and the table do,
        once).  Synchronises `stream` (None: the current torch stream)."""
        import torch
        for a, dt, name in ((row_ptr, torch.int32, "row_ptr"), (col_idx, torch.int32, "col_idx"),
                            (ids, torch.uint8, "ids"), (table, torch.float32, "table")):
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise TypeError(f"{name} must be a CUDA (HIP) torch tensor")
            if a.dtype != dt:
                raise TypeError(f"{name} must be {dt}")
            if a.device.index != device:
                raise ValueError(f"{name} must be on device {device}")
        rp, ci = row_ptr.contiguous().reshape(-1), col_idx.contiguous().reshape(-1)
        idv, tb = ids.contiguous().reshape(-1), table.contiguous().reshape(-1)
        if rp.numel() < 1:
            raise ValueError("row_ptr needs n_rows + 1 elements")
        if idv.numel() != ci.numel():
            raise ValueError(f"ids has {idv.numel()} elements, col_idx {ci.numel()}")
        if tb.numel() > 255 or (ci.numel() > 0 and tb.numel() < 1):
            raise ValueError(f"table must hold 1..255 values, got {tb.numel()}")
        return cls._created(device, _lib.load().sm_create_from_csr_ids_device,
                            (int(rp.numel()) - 1, n_cols, int(ci.numel()), _ptr(rp), _ptr(ci), _ptr(idv), _ptr(tb),
                             int(tb.numel()), device, _stream_of(rp, stream)), opts, (), "from_csr_ids_device")

    # ---- the transposed matrix ---------------------------------------------
    def transposed(self, opts: Optional[dict] = None, stream=None) -> "SparseMatrix":
        """A new, independent SparseMatrix holding B^T (sm_create_transpose): transposed on the
        device from this matrix's device CSR -- row c of B^T holds column c's terms by ascending
        source row, values bit for bit.  `opts`: the fields of sm_build_opts, as for from_csr
        (None: the constructors' defaults).  A CopyForm-built matrix gives what CopyForm builds
        from the same index with the other `trans` (without the reference stream:
        build_ref_stream adds it).  Synchronises `stream` (None: the current torch stream)."""
        h0 = self._require()
        if self._updatable():   # the companion of an updatable matrix follows its updates
            opts = dict(opts or {}, updatable=1)
        if self._table_updatable():
            opts = dict(opts or {}, table_updatable=1)
        return SparseMatrix._created(self.device, self._L.sm_create_transpose, (h0,), opts,
                                     (_stream_of(self, stream),), "transposed")

    @property
    def T(self) -> "SparseMatrix":
        """The transposed companion, built on first use (transposed() with default options)
        and cached until CopyForm or Destroy.  It is a second matrix on the device: holding it
        doubles the device memory held.  ``m.T.T`` is a third matrix equal to ``m`` (``==``),
        not ``m`` itself."""
        self._require()
        if self._t is None:
            self._t = self.transposed()
        return self._t

    def spmv_t(self, x, y, alpha: float = 1.0, beta: float = 1.0, algo="auto", stream=None):
        """y = alpha * B^T * x + beta * y on device tensors: spmv on the cached companion T
        (x: n_rows elements, y: n_cols elements of this matrix)."""
        return self.T.spmv(x, y, alpha, beta, algo, stream)

    def spmm_t(self, X, Y, alpha: float = 1.0, beta: float = 1.0, algo="auto", stream=None):
        """Y (k x N) = alpha * B^T * X (n x N) + beta * Y, row-major device tensors: spmm on
        the cached companion T."""
        return self.T.spmm(X, Y, alpha, beta, algo, stream)

    # ---- queries ----------------------------------------------------------
    def NumRows(self) -> int:
        """rows_ = k of the S view (sparse-matrix.h:39)."""
        return int(self._L.sm_num_rows(self._h)) if self._h else 0

    def NumCols(self) -> int:
        """cols_ = n of the S view (sparse-matrix.h:40)."""
        return int(self._L.sm_num_cols(self._h)) if self._h else 0

    def info(self) -> dict:
        inf = SmInfo()
        check(self._L.sm_get_info_ex(self._require(), C.byref(inf), C.sizeof(inf)), "sm_get_info")
        return {k: getattr(inf, k) for k, _ in SmInfo._fields_}

    def layout_digest(self) -> tuple:
        """sm_layout_digest: FNV-1a digests of the relabeling, the sliced ELL's structure, its
        slots and its codebook, or of a band layout's geometry, entries and table (0 where not
        built)."""
        d = (C.c_uint64 * 4)()
        check(self._L.sm_layout_digest(self._require(), d), "sm_layout_digest")
        return tuple(int(v) for v in d)

    def built_on_device(self) -> int:
        """sm_built_on_device: which layouts the device builders made -- 1 the column relabeling,
        2 the sliced ELL, 4 the gathered chunk bands, 8 the merge staging copy, 16 the balanced
        bands (band2, cband); 0 when the host builders made them all."""
        mask = C.c_uint32(0)
        check(self._L.sm_built_on_device(self._require(), C.byref(mask)), "sm_built_on_device")
        return int(mask.value)

    @property
    def n_rows(self) -> int:
        return self.info()["n_rows"]

    @property
    def n_cols(self) -> int:
        return self.info()["n_cols"]

    @property
    def nnz(self) -> int:
        return self.info()["nnz"]

    def csr(self):
        """Host copy of the device CSR of B: (row_ptr, col_idx, val)."""
        inf = self.info()
        rp = np.zeros(inf["n_rows"] + 1, np.int32)
        ci = np.zeros(max(inf["nnz"], 1), np.int32)
        va = np.zeros(max(inf["nnz"], 1), np.float32)
        check(self._L.sm_copy_csr(self._h, _ptr(rp), _ptr(ci), _ptr(va)), "sm_copy_csr")
        return rp, ci[: inf["nnz"]], va[: inf["nnz"]]

    def build_ref_stream(self, table: Optional[np.ndarray] = None) -> None:
        """Encode a CSR-built matrix in the reference's format (sm_build_ref_stream,
        sparse-matrix.cc:20-99): afterwards ref_stream(), == and algo="native" serve it.
        `table`: the codebook (<= 255 fp32 values every value must match); None takes the
        values' distinct bit patterns in CSR order.  On the transposed() of a CopyForm-built
        matrix, that matrix's own codebook gives the stream CopyForm builds with the other
        `trans` (the terms keep the ids the index gave them)."""
        if table is None:
            check(self._L.sm_build_ref_stream(self._h, None, 0), "sm_build_ref_stream")
            return
        tb = np.ascontiguousarray(table, np.float32)
        check(self._L.sm_build_ref_stream(self._h, _ptr(tb), int(tb.size)), "sm_build_ref_stream")

    def ref_stream(self) -> dict:
        """The reference encoding (pos_index_, val_index_, block bounds)."""
        inf = self.info()
        E, P = inf["n_entries"], inf["n_panels"]
        pos = np.zeros(max(E, 1), np.uint8)
        val = np.zeros(max(E, 1), np.uint8)
        ro = np.zeros(max(P, 1), np.int32)
        co = np.zeros(max(P, 1), np.int32)
        b = np.zeros(max(P, 1), np.int64)
        e = np.zeros(max(P, 1), np.int64)
        check(self._L.sm_copy_ref_stream(self._h, _ptr(pos), _ptr(val), _ptr(ro), _ptr(co),
                                         _ptr(b), _ptr(e)), "sm_copy_ref_stream")
        return dict(rows=inf["s_rows"], cols=inf["s_cols"], pos=pos[:E], val=val[:E],
                    panel_row_off=ro[:P], panel_col_off=co[:P], panel_begin=b[:P],
                    panel_end=e[:P])

    def CopyTo(self, density_matrix: Optional[np.ndarray], stride: int,
               trans: int = SblasNoTrans) -> np.ndarray:
        """sparse-matrix.cc:101-137: decode into a dense float matrix (host).  NoTrans (the
        default) writes S, Trans writes S^T = B; dense_device below is the device form, whose
        default is the other way round: B."""
        inf = self.info()
        nr = inf["s_cols"] if trans else inf["s_rows"]
        if density_matrix is None:
            density_matrix = np.zeros(max(nr * stride, 1), np.float32)
        out = density_matrix
        if not (isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous):
            raise TypeError("CopyTo needs a C-contiguous float32 numpy array")
        if out.size < nr * stride:
            raise ValueError("output smaller than rows * stride")
        check(self._L.sm_to_dense(self._h, _ptr(out), stride, int(trans)), "CopyTo")
        return out

    def dense_device(self, out=None, trans: bool = True, stream=None):
        """CopyTo with a device output (sm_to_dense_device).  Mind the orientation: CopyTo's
        default (NoTrans) is the reference's S view, this method's default (``trans=True``) is
        B = S^T, the ``n_rows x n_cols`` matrix from_csr and from_dense take, so that
        ``from_dense(M.dense_device(), ...)`` round-trips; ``trans=False`` gives the S view
        (``n_cols x n_rows``).  `out`: None for a new tensor, or a 2-D float32 tensor on the
        matrix's device with ``stride(1) == 1`` and at least that many rows and columns (a padded
        or row-sliced view is fine): the leading rows x columns are written in place -- zeros where
        nothing is stored -- and its padding stays untouched.  A (row, column) stored more than
        once gets its last stored term's value.  Asynchronous on `stream` (None: the current torch
        stream); nothing is allocated by the library, so the call can be captured in a graph."""
        import torch
        h = self._require()
        n_rows, n_cols = self._dims()
        rows, cols = (n_rows, n_cols) if trans else (n_cols, n_rows)
        if out is None:
            out = torch.empty((rows, cols), dtype=torch.float32, device=torch.device("cuda", self.device))
        else:
            _check_dev_2d(out, rows, cols, "out")
            if out.device.index != self.device:
                raise ValueError("out must be on the matrix's device")
        ld = int(out.stride(0)) if out.shape[0] > 1 else max(cols, 1)
        if rows and cols:
            st = self._L.sm_to_dense_device(h, _ptr(out), ld, SM_TRANS if trans else SM_NO_TRANS,
                                            _stream_of(out, stream))
            check(st, "dense_device")
        return out

    def __eq__(self, other) -> bool:
        """operator== (sparse-matrix.cc:197-207)."""
        if not isinstance(other, SparseMatrix):
            return NotImplemented
        if not self._h or not other._h:
            return not self._h and not other._h
        return bool(self._L.sm_equal(self._h, other._h))

    __hash__ = None

    # ---- compute ------------------------------------------------------------
    def AddMatMat(self, a, m: int, lda: int, c, ldc: int, alpha: float, beta: float,
                  algo="parity", stream=None):
        """sparse-matrix.cc:139-194: C (m x n) = alpha * A (m x k) * S + beta * C, in place.

        numpy operands: synchronous and bit-identical to the reference.
        torch cuda operands: asynchronous on the current stream with `algo`."""
        h = self._require()
        k, n = self.NumRows(), self.NumCols()
        need_a = (m - 1) * lda + k if (m > 0 and alpha != 0.0 and k > 0) else 0
        need_c = (m - 1) * ldc + n if (m > 0 and n > 0) else 0
        if _is_device(c):
            _check_dev(c, need_c, "c")
            if need_a:
                _check_dev(a, need_a, "a")
            st = self._L.sm_addmatmat(h, _ptr(a), m, lda, _ptr(c), ldc, alpha, beta, _algo(algo),
                                      _stream_of(c, stream))
        else:
            if not (isinstance(c, np.ndarray) and c.dtype == np.float32 and c.flags.c_contiguous):
                raise TypeError("host AddMatMat needs C-contiguous float32 numpy arrays")
            a_arr = np.ascontiguousarray(a, np.float32)
            if c.size < need_c or a_arr.size < need_a:
                raise ValueError("a or c smaller than the (m, lda/ldc) layout requires")
            st = self._L.sm_addmatmat_host(h, _ptr(a_arr), m, lda, _ptr(c), ldc, alpha, beta)
        check(st, "AddMatMat")
        return c

    def spmv(self, x, y, alpha: float = 1.0, beta: float = 1.0, algo="auto", stream=None):
        """y = alpha * B * x + beta * y on device tensors (float32, contiguous)."""
        n_rows, n_cols = self._dims()
        _check_dev(x, n_cols, "x")
        _check_dev(y, n_rows, "y")
        if (x.dim() != 1 and not x.is_contiguous()) or (y.dim() != 1 and not y.is_contiguous()):
            raise ValueError("x and y must be contiguous")
        if x.dim() == 1 and x.stride(0) != 1 or y.dim() == 1 and y.stride(0) != 1:
            raise ValueError("x and y must be unit-stride")
        st = self._L.sm_spmv(self._require(), alpha, _ptr(x), beta, _ptr(y), _algo(algo),
                             _stream_of(y, stream))
        check(st, "sm_spmv")
        return y

    def spmm(self, X, Y, alpha: float = 1.0, beta: float = 1.0, algo="auto", stream=None):
        """Y (n x N) = alpha * B * X (k x N) + beta * Y, row-major device tensors."""
        n_rhs = int(Y.shape[1])
        n_rows, n_cols = self._dims()
        _check_dev_2d(X, n_cols, n_rhs, "X")
        _check_dev_2d(Y, n_rows, n_rhs, "Y")
        st = self._L.sm_spmm(self._require(), n_rhs, alpha, _ptr(X), int(X.stride(0)), beta,
                             _ptr(Y), int(Y.stride(0)), _algo(algo), _stream_of(Y, stream))
        check(st, "sm_spmm")
        return Y

    def sddmm(self, G, X, out=None, alpha: float = 1.0, beta: float = 0.0, algo="auto",
              stream=None):
        """out[e] = alpha * <G[r_e, :], X[c_e, :]> + beta * out[e] for every stored term e of B
        in CSR order (sm_sddmm): with G = dL/dY, the gradient of the stored values of
        Y = alpha * B * X.  G (n_rows x N) and X (n_cols x N) are float32 device tensors, row-major
        with stride(1) == 1 and any stride(0) >= N; 1-D G and X of n_rows / n_cols elements mean
        N = 1.  `out`: nnz float32 elements, contiguous; None allocates zeros (beta scales what
        is there, so uninitialised memory will not do).  Returns `out`."""
        import torch
        n_rows, n_cols = self._dims()
        h = self._require()
        nnz = self._nnz()
        n_rhs, ldg = _sddmm_operand(G, n_rows, "G")
        n_x, ldx = _sddmm_operand(X, n_cols, "X")
        if n_x != n_rhs:
            raise ValueError(f"G has {n_rhs} columns, X has {n_x}")
        if n_rhs < 1:
            raise ValueError("G and X need at least one column")
        if G.device != X.device:
            raise ValueError("G and X must be on the same device")
        if out is None:
            out = torch.zeros(nnz, dtype=torch.float32, device=G.device)
        else:
            _check_dev(out, nnz, "out")
            if out.dim() != 1 or out.numel() != nnz or (nnz > 1 and out.stride(0) != 1):
                raise ValueError(f"out must be a unit-stride 1-D tensor of nnz = {nnz} elements")
            if out.device != G.device:
                raise ValueError("out must be on the device of G and X")
        st = self._L.sm_sddmm(h, n_rhs, alpha, _ptr(G), ldg, _ptr(X), ldx, beta, _ptr(out),
                              _algo(algo), _stream_of(out, stream))
        check(st, "sm_sddmm")
        return out

    def _nnz(self) -> int:
        """nnz of the held matrix, cached per handle like _dims."""
        h = self._require()
        if getattr(self, "_nnz_h", None) != h:
            inf = self.info()
            self._nnz_cache = inf["nnz"]
            self._upd_cache = bool(inf["updatable"])
            self._tupd_cache = bool(inf["table_updatable"])
            self._tsize_cache = inf["table_size"]
            self._nnz_h = h
        return self._nnz_cache

    def _table_updatable(self) -> bool:
        """Built with opts table_updatable=1 (cached per handle like _nnz)."""
        self._nnz()
        return self._tupd_cache

    def _table_size(self) -> int:
        self._nnz()
        return self._tsize_cache

    def _updatable(self) -> bool:
        """Built with opts updatable=1 (cached per handle like _nnz)."""
        self._nnz()
        return self._upd_cache

    # ---- updating the stored values in place ----------------------------------
    def _values_operand(self, t, name: str) -> None:
        nnz = self._nnz()
        _check_dev(t, nnz, name)
        if t.dim() != 1 or t.numel() != nnz or (nnz > 1 and t.stride(0) != 1):
            raise ValueError(f"{name} must be a unit-stride 1-D tensor of nnz = {nnz} elements")
        if t.device.index != self.device:
            raise ValueError(f"{name} must be on the matrix's device")

    def set_values(self, val, stream=None) -> None:
        """val[e] = val_new[e], bit for bit, for every stored term e in CSR order (sm_set_values),
        on a matrix built with ``opts={"updatable": 1}``: afterwards the matrix is what from_csr
        builds from the new values with the same options, every layout and product bit for bit.
        `val`: nnz float32 elements on the matrix's device.  Asynchronous on `stream` (None: the
        current torch stream), no allocation and no synchronisation, so it can be captured in a
        graph.  A cached transposed companion (T) is updated on the same stream.  The call writes
        the matrix: order it against products of this matrix on other streams."""
        h = self._require()
        self._values_operand(val, "val")
        s = _stream_of(self, stream)
        check(self._L.sm_set_values(h, _ptr(val), _lib.SM_VALUES_OWN, s), "sm_set_values")
        if self._t is not None:
            check(self._L.sm_set_values(self._t._require(), _ptr(val), _lib.SM_VALUES_SOURCE, s),
                  "sm_set_values (T)")

    def axpy_values(self, a: float, delta, stream=None) -> None:
        """val[e] = fl(val[e] + fl(a * delta[e])) for every stored term e in CSR order
        (sm_axpy_values; two roundings, no fused multiply-add), on a matrix built with
        ``opts={"updatable": 1}`` -- an optimiser step on the values, e.g.
        ``m.axpy_values(-lr, grad)`` with the gradient sddmm gives.  a == 0 does nothing and
        `delta` may then be None.  Stream behaviour and the companion T as for set_values."""
        h = self._require()
        a = float(a)
        if a != 0.0 or delta is not None:
            self._values_operand(delta, "delta")
        s = _stream_of(self, stream)
        check(self._L.sm_axpy_values(h, a, _ptr(delta), _lib.SM_VALUES_OWN, s), "sm_axpy_values")
        if self._t is not None:
            check(self._L.sm_axpy_values(self._t._require(), a, _ptr(delta), _lib.SM_VALUES_SOURCE, s),
                  "sm_axpy_values (T)")

    # ---- table matrices (from_csr_ids): table gradient and in-place table updates ----------
    def table_device(self, stream=None):
        """The current table of a table matrix as a new float32 tensor of T elements on its
        device (sm_copy_table_device), copied on `stream` (None: the current torch stream)."""
        import torch
        h = self._require()
        t = torch.empty(self._table_size(), dtype=torch.float32, device=torch.device("cuda", self.device))
        check(self._L.sm_copy_table_device(h, _ptr(t) if t.numel() else 0, _stream_of(t, stream)),
              "sm_copy_table_device")
        return t

    def term_ids_device(self, stream=None):
        """The terms' ids of a table matrix in CSR order, a new uint8 tensor of nnz elements on
        its device (sm_copy_term_ids_device)."""
        import torch
        h = self._require()
        t = torch.empty(self._nnz(), dtype=torch.uint8, device=torch.device("cuda", self.device))
        check(self._L.sm_copy_term_ids_device(h, _ptr(t) if t.numel() else 0, _stream_of(t, stream)),
              "sm_copy_term_ids_device")
        return t

    def sddmm_table(self, G, X, out=None, alpha: float = 1.0, beta: float = 0.0, algo="auto",
                    stream=None):
        """out[t] = alpha * sum over the terms e with id t of <G[r_e, :], X[c_e, :]> + beta * out[t]
        (sm_sddmm_table): with G = dL/dY, the gradient of the table of Y = alpha * B * X, in one
        deterministic fused pass (no nnz-sized array).  G and X as for sddmm; alpha == 0 takes
        G = X = None.  `out`: T float32 elements on the matrix's device (any 4-byte alignment);
        None allocates zeros.  Returns `out`."""
        import torch
        n_rows, n_cols = self._dims()
        h = self._require()
        T = self._table_size()
        if alpha == 0.0 and G is None and X is None:
            n_rhs, ldg, ldx = 1, 1, 1
        else:
            n_rhs, ldg = _sddmm_operand(G, n_rows, "G")
            n_x, ldx = _sddmm_operand(X, n_cols, "X")
            if n_x != n_rhs:
                raise ValueError(f"G has {n_rhs} columns, X has {n_x}")
            if n_rhs < 1:
                raise ValueError("G and X need at least one column")
            if G.device != X.device:
                raise ValueError("G and X must be on the same device")
        if out is None:
            out = torch.zeros(T, dtype=torch.float32, device=torch.device("cuda", self.device))
        else:
            self._table_operand(out, "out")
        st = self._L.sm_sddmm_table(h, n_rhs, alpha, _ptr(G), ldg, _ptr(X), ldx, beta, _ptr(out),
                                    _algo(algo), _stream_of(out, stream))
        check(st, "sm_sddmm_table")
        return out

    def _table_operand(self, t, name: str) -> None:
        T = self._table_size()
        _check_dev(t, T, name)
        if T == 0:   # not a table matrix (or an empty one): the library answers
            return
        if t.dim() != 1 or t.numel() != T or (T > 1 and t.stride(0) != 1):
            raise ValueError(f"{name} must be a unit-stride 1-D tensor of T = {T} elements")
        if t.device.index != self.device:
            raise ValueError(f"{name} must be on the matrix's device")

    def set_table(self, t, stream=None) -> None:
        """table[i] = t[i], bit for bit (sm_set_table), on a matrix built by from_csr_ids with
        ``opts={"table_updatable": 1}``: afterwards the matrix is what from_csr_ids builds from the
        same pattern and ids with the new table, every layout and product bit for bit.  `t`: T
        float32 elements on the matrix's device.  Asynchronous on `stream`, capturable; a cached
        transposed companion (T) takes the same call on the same stream.  The call writes the
        matrix: order it against products of this matrix on other streams."""
        h = self._require()
        self._table_operand(t, "t")
        s = _stream_of(self, stream)
        check(self._L.sm_set_table(h, _ptr(t), s), "sm_set_table")
        if self._t is not None:
            check(self._L.sm_set_table(self._t._require(), _ptr(t), s), "sm_set_table (T)")

    def axpy_table(self, a: float, delta, stream=None) -> None:
        """table[i] = fl(table[i] + fl(a * delta[i])) (sm_axpy_table; two roundings, no fused
        multiply-add) -- an optimiser step on the table, e.g. ``m.axpy_table(-lr, grad)`` with the
        gradient sddmm_table gives.  a == 0 does nothing and `delta` may then be None.  Stream
        behaviour and the companion T as for set_table."""
        h = self._require()
        a = float(a)
        if a != 0.0 or delta is not None:
            self._table_operand(delta, "delta")
        s = _stream_of(self, stream)
        check(self._L.sm_axpy_table(h, a, _ptr(delta), s), "sm_axpy_table")
        if self._t is not None:
            check(self._L.sm_axpy_table(self._t._require(), a, _ptr(delta), s), "sm_axpy_table (T)")

    # ---- quantising the stored values: k-means on the device ---------------------------------
    def _codebook_operand(self, t, name: str) -> int:
        """T of a table operand of the quantiser: 1..255 float32 elements on the matrix's device."""
        _check_dev(t, 1, name)
        if t.dim() != 1 or t.numel() > 255 or (t.numel() > 1 and t.stride(0) != 1):
            raise ValueError(f"{name} must be a unit-stride 1-D tensor of 1..255 elements")
        if t.device.index != self.device:
            raise ValueError(f"{name} must be on the matrix's device")
        return int(t.numel())

    def quantize_assign(self, table, stream=None):
        """ids[e] = the entry of `table` nearest to the stored value of term e (sm_quantize_assign;
        the header states the tie rule), for the stored values of any matrix: a new uint8 tensor of
        nnz elements on the matrix's device.  `table`: 1..255 float32 elements on that device.
        Synchronises `stream` (None: the current torch stream)."""
        import torch
        h = self._require()
        T = self._codebook_operand(table, "table")
        ids = torch.empty(self._nnz(), dtype=torch.uint8, device=torch.device("cuda", self.device))
        st = self._L.sm_quantize_assign(h, _ptr(table), T, _ptr(ids) if ids.numel() else 0,
                                        _stream_of(ids, stream))
        check(st, "sm_quantize_assign")
        return ids

    def quantize_update(self, ids, table, stream=None):
        """One Lloyd update (sm_quantize_update): table[t] <- the mean of the stored values with id
        t, in place (an id with no value keeps its entry), summed in double in the header's fixed
        order.  `ids`: nnz uint8 elements, `table`: 1..255 float32 elements, both on the matrix's
        device.  Returns (counts, sse): an int32 tensor of T elements and the sum of squared
        distances to the OLD table as a float64 tensor of one element.  Synchronises `stream`."""
        import torch
        h = self._require()
        T = self._codebook_operand(table, "table")
        nnz = self._nnz()
        if not isinstance(ids, torch.Tensor) or not ids.is_cuda or ids.dtype != torch.uint8:
            raise TypeError("ids must be a CUDA (HIP) uint8 torch tensor")
        if ids.dim() != 1 or ids.numel() != nnz or (nnz > 1 and ids.stride(0) != 1):
            raise ValueError(f"ids must be a unit-stride 1-D tensor of nnz = {nnz} elements")
        if ids.device.index != self.device:
            raise ValueError("ids must be on the matrix's device")
        dev = torch.device("cuda", self.device)
        counts = torch.empty(T, dtype=torch.int32, device=dev)
        sse = torch.empty(1, dtype=torch.float64, device=dev)
        st = self._L.sm_quantize_update(h, _ptr(ids) if nnz else 0, T, _ptr(table), _ptr(counts), _ptr(sse),
                                        _stream_of(table, stream))
        check(st, "sm_quantize_update")
        return counts, sse

    def quantized(self, table_size: int = 255, iters: int = 8, init=None, opts: Optional[dict] = None,
                  stream=None) -> "SparseMatrix":
        """A new table matrix with this matrix's pattern and its stored values quantised to
        `table_size` <= 255 shared values by `iters` k-means (Lloyd) steps on the device
        (sm_create_quantized): the start is `init` (table_size float32 elements on the matrix's
        device) or, for None, the linear table between the least and greatest value.  This matrix
        is only read.  `opts`: as for from_csr_ids -- ``{"table_updatable": 1}`` for fine-tuning the
        table with sddmm_table / axpy_table.  A NaN or Inf value raises (invalid matrix).
        Synchronises `stream` (None: the current torch stream)."""
        h0 = self._require()
        table_size, iters = int(table_size), int(iters)
        if init is not None and self._codebook_operand(init, "init") != table_size:
            raise ValueError(f"init must hold table_size = {table_size} elements")
        return SparseMatrix._created(self.device, self._L.sm_create_quantized, (h0, table_size, iters, _ptr(init)), opts,
                                     (_stream_of(self, stream),), "quantized")

    # ---- pruning the stored terms by magnitude: mask, compact, rebuild ------------------------
    @staticmethod
    def _prune_args(keep, per_row, threshold):
        """(mode, count, threshold) of the C ABI from the three exclusive keyword arguments."""
        if sum(a is not None for a in (keep, per_row, threshold)) != 1:
            raise ValueError("give exactly one of keep, per_row and threshold")
        if keep is not None:
            return _lib.SM_PRUNE_GLOBAL_TOPK, int(keep), 0.0
        if per_row is not None:
            return _lib.SM_PRUNE_ROW_TOPK, int(per_row), 0.0
        return _lib.SM_PRUNE_THRESHOLD, 0, float(threshold)

    def prune_mask(self, keep=None, per_row=None, threshold=None, stream=None):
        """The mask of the terms to keep (sm_prune_mask; the header states the rule on the values'
        bits): a new uint8 tensor of nnz ones and zeros in CSR order on the matrix's device, for the
        stored values of any matrix.  Exactly one of `keep` (the number of terms of greatest |value|
        of the whole matrix), `per_row` (of every row) and `threshold` (keep |value| >= threshold).
        Ties go to the earlier stored term; a NaN is kept first.  Synchronises `stream` (None: the
        current torch stream)."""
        import torch
        h = self._require()
        mode, count, thr = self._prune_args(keep, per_row, threshold)
        mask = torch.empty(self._nnz(), dtype=torch.uint8, device=torch.device("cuda", self.device))
        st = self._L.sm_prune_mask(h, mode, count, thr, _ptr(mask) if mask.numel() else 0, None,
                                   _stream_of(mask, stream))
        check(st, "sm_prune_mask")
        return mask

    def masked(self, keep, opts: Optional[dict] = None, stream=None) -> "SparseMatrix":
        """A new, independent matrix holding the terms whose keep[e] != 0, in stored order
        (sm_create_masked), compacted on the device; the layouts are those from_csr builds from the
        compacted arrays with the same `opts`.  `keep`: nnz uint8 elements on the matrix's device.
        A table matrix gives a table matrix (same table, the kept terms' ids).  The result remembers
        every term's index in this matrix (source_terms_device); built with
        ``opts={"updatable": 1}`` it takes values laid out for this matrix (sm_set_values with
        SM_VALUES_SOURCE).  Synchronises `stream` (None: the current torch stream)."""
        import torch
        h0 = self._require()
        nnz = self._nnz()
        if not isinstance(keep, torch.Tensor) or not keep.is_cuda or keep.dtype != torch.uint8:
            raise TypeError("keep must be a CUDA (HIP) uint8 torch tensor")
        if keep.dim() != 1 or keep.numel() != nnz or (nnz > 1 and keep.stride(0) != 1):
            raise ValueError(f"keep must be a unit-stride 1-D tensor of nnz = {nnz} elements")
        if keep.device.index != self.device:
            raise ValueError("keep must be on the matrix's device")
        return SparseMatrix._created(self.device, self._L.sm_create_masked, (h0, _ptr(keep) if nnz else 0), opts,
                                     (_stream_of(self, stream),), "masked")

    def pruned(self, keep=None, per_row=None, threshold=None, opts: Optional[dict] = None,
               stream=None) -> "SparseMatrix":
        """prune_mask, then masked, without the mask leaving the library (sm_create_pruned):
        ``P = M.pruned(keep=M.nnz // 2, opts={"updatable": 1})``.  Arguments as for those two."""
        h0 = self._require()
        mode, count, thr = self._prune_args(keep, per_row, threshold)
        return SparseMatrix._created(self.device, self._L.sm_create_pruned, (h0, mode, count, thr), opts,
                                     (_stream_of(self, stream),), "pruned")

    def source_terms_device(self, stream=None):
        """For a matrix made by masked / pruned (or transposed with ``opts={"updatable": 1}``):
        terms[e] = the CSR index, in the matrix it was made from, of this matrix's term e
        (sm_copy_source_terms_device) -- a new int32 tensor of nnz elements on the matrix's device,
        copied on `stream`.  ``state[terms.long()]`` gathers per-term state of the source."""
        import torch
        h = self._require()
        t = torch.empty(self._nnz(), dtype=torch.int32, device=torch.device("cuda", self.device))
        check(self._L.sm_copy_source_terms_device(h, _ptr(t) if t.numel() else 0, _stream_of(t, stream)),
              "sm_copy_source_terms_device")
        return t

    # ---- the sum of two matrices on the union of their patterns --------------------------------
    def sum(self, other: "SparseMatrix", alpha: float = 1.0, beta: float = 1.0, opts: Optional[dict] = None,
            stream=None) -> "SparseMatrix":
        """``alpha * self + beta * other`` as a new, independent matrix on the union of the two
        patterns (sm_create_sum; the header states the value rule bit for bit): every row holds the
        union of the two rows' columns, ascending; a term is kept whatever its value; a coefficient
        of 0 leaves that operand's values unread and one of 1 takes them as they are, so
        ``A.sum(G, 1, 0)`` is A on the union pattern with the new positions at +0.0 (the regrow step
        of dynamic sparse training).  Both operands' rows must strictly ascend, and they must share
        shape and device; `other` may be `self`.  The layouts are those from_csr builds from the
        summed arrays with the same `opts`; the result remembers where every term came from
        (sum_terms_device).  Synchronises `stream` (None: the current torch stream)."""
        h0 = self._require()
        if not isinstance(other, SparseMatrix):
            raise TypeError("other must be a SparseMatrix")
        h1 = other._require()
        return SparseMatrix._created(self.device, self._L.sm_create_sum, (h0, float(alpha), h1, float(beta)), opts,
                                     (_stream_of(self, stream),), "sum")

    def sum_terms_device(self, stream=None):
        """For a matrix made by sum: ``(terms_a, terms_b)``, two new int32 tensors of nnz elements on
        the matrix's device, copied on `stream` (sm_copy_sum_terms_device).  terms_a[e] is the CSR
        index, in the first operand, of this matrix's term e, or -1 where that operand does not
        store the position; terms_b the same for the second operand."""
        import torch
        h = self._require()
        dev = torch.device("cuda", self.device)
        n = self._nnz()
        ta = torch.empty(n, dtype=torch.int32, device=dev)
        tb = torch.empty(n, dtype=torch.int32, device=dev)
        check(self._L.sm_copy_sum_terms_device(h, _ptr(ta) if n else 0, _ptr(tb) if n else 0, _stream_of(ta, stream)),
              "sm_copy_sum_terms_device")
        return ta, tb

    def csr_device(self, stream=None):
        """(row_ptr, col_idx, val): new torch tensors on the matrix's device holding its CSR
        (sm_copy_csr_device; int32, int32, float32), copied on `stream` (None: the current
        torch stream).  ``from_csr(row_ptr, col_idx, new_val, n_cols)`` takes them back, so
        values can be updated without a host round trip; a matrix built with
        ``opts={"updatable": 1}`` takes them in place instead (set_values, axpy_values)."""
        import torch
        inf = self.info()
        dev = torch.device("cuda", self.device)
        rp = torch.empty(inf["n_rows"] + 1, dtype=torch.int32, device=dev)
        ci = torch.empty(inf["nnz"], dtype=torch.int32, device=dev)
        va = torch.empty(inf["nnz"], dtype=torch.float32, device=dev)
        st = self._L.sm_copy_csr_device(self._h, _ptr(rp), _ptr(ci) if inf["nnz"] else 0,
                                        _ptr(va) if inf["nnz"] else 0, _stream_of(rp, stream))
        check(st, "sm_copy_csr_device")
        return rp, ci, va

    # ---- the reference's own known-answer test -------------------------------
    @staticmethod
    def SelfTest(device: int = 0, seed: int = 0) -> bool:
        """sparse-matrix.cc:209-313, run through this library: the two 3x2/2x3 KATs and
        a 1023 x 511 (stride 512) NoTrans/Trans round trip at 25 % density."""
        table8 = np.array([1.1, 2.2, 3.3, 4.4, 5.5, 6.6, 7.7, 8.8], np.float32)
        want = np.array([1.1, 0, 0, 4.4, 8.8, 0], np.float32)
        for dm, rows, cols, stride, trans in (
                (np.array([0, 255, 255, 3, 7, 255], np.uint8), 3, 2, 2, SblasNoTrans),
                (np.array([0, 255, 7, 255, 3, 255], np.uint8), 2, 3, 3, SblasTrans)):
            sm = SparseMatrix(dm, rows, cols, stride, table8, 8, trans, device=device)
            out = np.ones(6, np.float32)
            sm.CopyTo(out, 2)
            if not np.array_equal(out, want):
                return False
            if trans:
                out = np.ones(6, np.float32)
                sm.CopyTo(out, stride, SblasTrans)
                if not np.array_equal(out, np.array([1.1, 0, 8.8, 0, 4.4, 0], np.float32)):
                    return False
            a = np.array([3.1, 5, 7], np.float32)
            c = np.array([4, 8], np.float32)
            sm.AddMatMat(a, 1, 3, c, 2, 1.3, 2.0)
            if abs(c[0] - 92.513) > 1e-3 or abs(c[1] - 44.6) > 1e-3:
                return False
        rng = np.random.default_rng(seed)
        m, n, stride = 1023, 511, 512
        live = np.zeros(m * stride, bool)
        live[rng.permutation(m * stride)[: m * stride - int(m * stride * 0.75)]] = True
        table = rng.uniform(-1000, 1000, 64).astype(np.float32)
        index = np.where(live, rng.integers(0, 63, m * stride), 255).astype(np.uint8)
        matrix = np.where(live, table[np.minimum(index, 63)], 0).astype(np.float32)
        sm = SparseMatrix(device=device)
        for trans in (SblasNoTrans, SblasTrans):
            sm.CopyForm(index, m, n, stride, table, 63, trans)
            copy = np.zeros(m * stride, np.float32)
            sm.CopyTo(copy, stride, trans)
            if not np.array_equal(matrix.reshape(m, stride)[:, :n], copy.reshape(m, stride)[:, :n]):
                return False
        return True


# ---- kernel.h helpers on device tensors (kernel.cc:10-187) ---------------------------
def sblas_beta_operation_kernel(c, m: int, n: int, ldc: int, beta: float, stream=None):
    L = _lib.load()
    check(L.sm_beta_scale(_ptr(c), m, n, ldc, beta, _stream_of(c, stream)), "sm_beta_scale")
    return c


def sblas_trans_kernel(a, m: int, n: int, lda: int, sa, ldsa: int, stream=None):
    L = _lib.load()
    check(L.sm_transpose(_ptr(a), m, n, lda, _ptr(sa), ldsa, _stream_of(sa, stream)),
          "sm_transpose")
    return sa
