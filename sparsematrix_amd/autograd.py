"""``Y = alpha * B * X`` as a differentiable torch op over a held SparseMatrix.

Plumbing only: the forward pass is the matrix's own ``spmv`` / ``spmm`` into a zeroed
output (beta = 0), the backward pass the same product on the cached transposed companion
``matrix.T`` (``grad_X = alpha * B^T * grad_Y``) and, for the stored values, the matrix's
``sddmm`` (``grad_values[e] = alpha * <grad_Y[r_e, :], X[c_e, :]>`` in CSR order).  All
arithmetic stays in the library's HIP kernels.

    from sparsematrix_amd import autograd
    Y = autograd.apply(m, X, alpha=1.3)     # X: n_cols (SpMV) or n_cols x N row-major (SpMM)
    Y.backward(G)                            # X.grad = 1.3 * m.T @ G

    rp, ci, val = m.csr_device()             # the stored values as a leaf
    val.requires_grad_()
    Y = autograd.apply(m, X, alpha=1.3, values=val)
    Y.backward(G)                            # val.grad = m.sddmm(G, X, alpha=1.3)

    tab = m.table_device().requires_grad_()  # a table matrix (from_csr_ids): its table as a leaf
    Y = autograd.apply_table(m, X, alpha=1.3, table=tab)
    Y.backward(G)                            # tab.grad = m.sddmm_table(G, X, alpha=1.3)
"""
from __future__ import annotations

_fn = None


def _product(matrix, X, alpha: float):
    """alpha * matrix * X into a zero-initialised output of X's rank."""
    import torch
    n_rows, n_cols = matrix._dims()
    if X.dim() not in (1, 2) or X.shape[0] != n_cols:
        raise ValueError(f"X must have {n_cols} elements (1-D) or {n_cols} rows (2-D), got {tuple(X.shape)}")
    if X.dim() == 1:
        Y = torch.zeros(n_rows, dtype=torch.float32, device=X.device)
        return matrix.spmv(X, Y, alpha, 0.0)
    Y = torch.zeros((n_rows, X.shape[1]), dtype=torch.float32, device=X.device)
    return matrix.spmm(X, Y, alpha, 0.0)


def _function():
    global _fn
    if _fn is not None:
        return _fn
    import torch
    from torch.autograd.function import once_differentiable

    class SparseMatMul(torch.autograd.Function):
        @staticmethod
        def forward(ctx, X, matrix, alpha, values, table):
            ctx.matrix, ctx.alpha = matrix, float(alpha)
            Xc = X.detach().contiguous()
            if values is not None and ctx.needs_input_grad[3]:
                ctx.values_shape = values.shape
                ctx.save_for_backward(Xc)   # X is kept only when the values want a gradient
            if table is not None and ctx.needs_input_grad[4]:
                ctx.table_shape = table.shape
                ctx.save_for_backward(Xc)   # ... or the table does
            return _product(matrix, Xc, ctx.alpha)

        @staticmethod
        @once_differentiable   # first-order only: a double backward raises instead of going wrong
        def backward(ctx, grad_Y):
            grad_X = grad_values = grad_table = None
            if ctx.needs_input_grad[0] or ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
                grad_Y = grad_Y.contiguous()
            if ctx.needs_input_grad[0]:
                grad_X = _product(ctx.matrix.T, grad_Y, ctx.alpha)
            if ctx.needs_input_grad[3]:
                (Xc,) = ctx.saved_tensors
                grad_values = ctx.matrix.sddmm(grad_Y, Xc, alpha=ctx.alpha).view(ctx.values_shape)
            if ctx.needs_input_grad[4]:
                (Xc,) = ctx.saved_tensors
                grad_table = ctx.matrix.sddmm_table(grad_Y, Xc, alpha=ctx.alpha).view(ctx.table_shape)
            return grad_X, None, None, grad_values, grad_table

    _fn = SparseMatMul
    return _fn


def apply(matrix, X, alpha: float = 1.0, values=None):
    """Y = alpha * B * X for the SparseMatrix `matrix` (B, n_rows x n_cols) and a float32 device
    tensor X of n_cols elements (1-D) or n_cols x N (row-major; made contiguous if it is not).
    Differentiable in X: backward computes alpha * B^T * grad_Y on ``matrix.T``, which is built
    on first use and doubles the device memory the matrix holds.

    `values` (optional): a float32 tensor of nnz elements on X's device that stands for the
    matrix's stored values, in CSR order, as the autograd leaf.  It must equal the matrix's
    current values (``matrix.csr_device()[2]``): the forward pass runs on the held matrix
    and never reads the tensor.  When it requires a gradient, backward returns
    ``matrix.sddmm(grad_Y, X, alpha=alpha)`` for it (X is saved for backward only then), and
    ``matrix.T`` is not built unless X requires a gradient too.  To step the values of a matrix
    built with ``opts={"updatable": 1}``, update it in place: ``matrix.axpy_values(-lr,
    values.grad)`` (a cached ``matrix.T`` follows on the same stream).  Then do the same to the
    leaf under ``torch.no_grad()`` -- ``values.add_(values.grad * -lr)``, the same two roundings,
    so the leaf stays equal bit for bit -- or re-read it from ``matrix.csr_device()[2]``.

    The table of a table matrix as the leaf: ``apply_table``."""
    return apply_table(matrix, X, alpha, values=values)


def apply_table(matrix, X, alpha: float = 1.0, table=None, values=None):
    """``apply`` with the table of a table matrix (``SparseMatrix.from_csr_ids``) as the leaf.

    `table` (optional, not together with `values`: ValueError): a float32 tensor of T elements on
    X's device that stands for the matrix's table (``matrix.table_device()``); never read in
    forward.  When it requires a gradient, backward returns
    ``matrix.sddmm_table(grad_Y, X, alpha=alpha)`` for it (X is saved only then).  The step on a
    matrix built with ``opts={"table_updatable": 1}``: ``matrix.axpy_table(-lr, table.grad)``,
    then under ``torch.no_grad()`` ``table.add_(table.grad * -lr)`` -- the same two roundings, so
    leaf and matrix stay equal bit for bit.  `values`, X and alpha as for ``apply`` (whose
    parameter list stays as it was; this is the entry that takes either leaf)."""
    if values is not None and table is not None:
        raise ValueError("values= and table= are two parametrisations of the same stored values: give one")
    if table is not None:
        import torch
        if not isinstance(table, torch.Tensor) or not table.is_cuda:
            raise TypeError("table must be a CUDA (HIP) torch tensor")
        if table.dtype != torch.float32:
            raise TypeError("table must be float32")
        if table.device != X.device:
            raise ValueError("table must be on X's device")
        T = matrix._table_size()
        if table.numel() != T:
            raise ValueError(f"table has {table.numel()} elements, the matrix's table {T}")
    if values is not None:
        import torch
        if not isinstance(values, torch.Tensor) or not values.is_cuda:
            raise TypeError("values must be a CUDA (HIP) torch tensor")
        if values.dtype != torch.float32:
            raise TypeError("values must be float32")
        if values.device != X.device:
            raise ValueError("values must be on X's device")
        nnz = matrix._nnz()
        if values.numel() != nnz:
            raise ValueError(f"values has {values.numel()} elements, the matrix stores {nnz} terms")
    return _function().apply(X, matrix, alpha, values, table)
