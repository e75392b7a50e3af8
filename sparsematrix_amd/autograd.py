"""``Y = alpha * B * X`` as a differentiable torch op over a held SparseMatrix.

Plumbing only: the forward pass is the matrix's own ``spmv`` / ``spmm`` into a zeroed
output (beta = 0), the backward pass the same product on the cached transposed companion
``matrix.T`` (``grad_X = alpha * B^T * grad_Y``).  All arithmetic stays in the library's HIP
kernels; the matrix itself gets no gradient.

    from sparsematrix_amd import autograd
    Y = autograd.apply(m, X, alpha=1.3)     # X: n_cols (SpMV) or n_cols x N row-major (SpMM)
    Y.backward(G)                            # X.grad = 1.3 * m.T @ G
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
        def forward(ctx, X, matrix, alpha):
            ctx.matrix, ctx.alpha = matrix, float(alpha)
            return _product(matrix, X.detach().contiguous(), ctx.alpha)

        @staticmethod
        @once_differentiable   # first-order only: a double backward raises instead of going wrong
        def backward(ctx, grad_Y):
            grad_X = None
            if ctx.needs_input_grad[0]:
                grad_X = _product(ctx.matrix.T, grad_Y.contiguous(), ctx.alpha)
            return grad_X, None, None

    _fn = SparseMatMul
    return _fn


def apply(matrix, X, alpha: float = 1.0):
    """Y = alpha * B * X for the SparseMatrix `matrix` (B, n_rows x n_cols) and a float32 device
    tensor X of n_cols elements (1-D) or n_cols x N (row-major; made contiguous if it is not).
    Differentiable in X: backward computes alpha * B^T * grad_Y on ``matrix.T``, which is built
    on first use and doubles the device memory the matrix holds."""
    return _function().apply(X, matrix, alpha)
