"""fp64 references and an arithmetic model of the lifter's graph kernels (csrc/graph_ops.hip).  TEST INFRASTRUCTURE ONLY.

Plain numpy / scipy, written from the definition of the operation (a K = 3 Chebyshev graph convolution, a CSR product,
feature-axis linear interpolation, a Linear on a few rows); nothing here calls the product.

  *_ref      fp64 on the operands the kernels see (fp32 inputs widened to fp64): what the GPU tests compare with
  *_model    the same operation in the kernels' arithmetic (fp32 gathers in CSR order, fp16 hi / lo split of basis and bank,
             hi*hi + hi*lo + lo*hi with fp32 accumulation): run on the CPU to show what error the arithmetic itself leaves
             and, with one cross term dropped, that the tests' bar can fail
  random_graph  seeded sparse square matrices whose row lengths sit on the gather-round boundaries of the fused kernel
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

# row lengths of random_graph: empty rows, both sides of the fused kernel's gather rounds (4, 8 and 16 neighbours of L per
# round), a long row and the mesh's own ~7
DEGREES = (0, 1, 4, 5, 8, 9, 16, 17, 40, 7)


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def random_graph(v: int, seed: int) -> sp.csr_matrix:
    """[v, v] fp32 CSR: row lengths cycle through DEGREES (capped at v) in a shuffled order, so every one of them occurs once
    v >= len(DEGREES); distinct random columns, sorted; signed values, every non-empty row scaled to absolute sum 1 (the
    spectrum stays inside the Chebyshev domain [-1, 1])."""
    rng = np.random.default_rng(seed)
    order = (1, 0) + tuple(d for d in DEGREES if d > 1)        # (a one-vertex graph keeps an entry, five vertices an empty row)
    deg = np.minimum(np.resize(np.asarray(order), v), v)
    rng.shuffle(deg)
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = np.empty(indptr[-1], np.int32)
    values = np.empty(indptr[-1], np.float64)
    for r in range(v):
        a, b = indptr[r], indptr[r + 1]
        if a == b:
            continue
        indices[a:b] = np.sort(rng.choice(v, size=b - a, replace=False))
        w = rng.uniform(0.2, 1.0, size=b - a) * rng.choice([-1.0, 1.0], size=b - a)
        values[a:b] = w / np.abs(w).sum()
    m = sp.csr_matrix((values.astype(np.float32), indices, indptr), shape=(v, v))
    m.has_sorted_indices = True
    return m


def cheby2(L: sp.csr_matrix) -> sp.csr_matrix:
    """2 L L - I: the product in fp64 on the fp32 coefficients, every coefficient rounded once to fp32, columns sorted."""
    m = L.tocsr().astype(np.float64)
    q = (2.0 * (m @ m) - sp.identity(m.shape[0], dtype=np.float64, format="csr")).tocsr()
    q.sum_duplicates()
    q.sort_indices()
    return q.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------
def spmm_ref(L: sp.csr_matrix, x: np.ndarray) -> np.ndarray:
    """x [B, V, F] -> L x per sample, fp64."""
    b, v, f = x.shape
    m = L.tocsr().astype(np.float64)
    return np.ascontiguousarray((m @ x.astype(np.float64).transpose(1, 0, 2).reshape(v, b * f)).reshape(v, b, f).transpose(1, 0, 2))


def basis_ref(L: sp.csr_matrix, x0: np.ndarray, x1: np.ndarray, cpad: int) -> np.ndarray:
    """[x0 | x1 | 2 L x1 - x0 | 0] as [B, V, cpad] fp64 (x1 is an INPUT of the basis kernel: L x0 as the caller computed it)."""
    b, v, f = x0.shape
    out = np.zeros((b, v, cpad), np.float64)
    out[..., :f] = x0
    out[..., f:2 * f] = x1
    out[..., 2 * f:3 * f] = 2.0 * spmm_ref(L, x1) - x0
    return out


def interp_weights(fi: int, fo: int, dtype=np.float64):
    """Linear interpolation from fi to fo samples with align_corners = False (ATen's source index: scale * (j + 0.5) - 0.5
    clamped at 0, scale = fi / fo; the upper neighbour clamped at fi - 1) -> i0 [fo], i1 [fo], w1 [fo]."""
    j = np.arange(fo, dtype=dtype)
    scale = dtype(fi) / dtype(fo)
    src = np.maximum(scale * (j + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(src.astype(np.int64), fi - 1)
    i1 = np.minimum(i0 + 1, fi - 1)
    return i0, i1, (src - i0.astype(dtype)).astype(dtype)


def feat_interp_add_ref(xin: np.ndarray, y: np.ndarray, up: int = 1) -> np.ndarray:
    """y [B, V, Fo] + interpolation of xin [B, V, Fi] along the feature axis, every row repeated `up` times; fp64."""
    i0, i1, w1 = interp_weights(xin.shape[2], y.shape[2])
    xi = xin.astype(np.float64)
    out = y.astype(np.float64) + (1.0 - w1) * xi[..., i0] + w1 * xi[..., i1]
    return np.repeat(out, up, axis=1)


def graph_conv_cheby3_ref(L, x, W, bias=None, relu=True, xin=None, up=1) -> np.ndarray:
    """One K = 3 Chebyshev graph convolution in fp64: act([x | L x | (2 L L - I) x] W^T + bias) (+ feature-axis interpolation
    of xin), rows repeated `up` times.  L: fp32 CSR; x [B, V, Fin]; W [Fout, 3 Fin] in k-major column order (fp32 values);
    the second-order matrix is cheby2(L), i.e. exactly the coefficients the kernel is given."""
    x64 = x.astype(np.float64)
    basis = np.concatenate([x64, spmm_ref(L, x), spmm_ref(cheby2(L), x)], axis=2)
    y = basis @ np.asarray(W, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if relu:
        y = np.maximum(y, 0.0)
    if xin is not None:
        return feat_interp_add_ref(xin, y, up)
    return np.repeat(y, up, axis=1)


def linear_rows_ref(x, W, bias=None, scale=None, shift=None, residual=None, relu=False) -> np.ndarray:
    """act(W pre(x) + bias (+ residual)) in fp64; pre = ReLU(x * scale + shift) when scale / shift are given."""
    a = np.asarray(x, np.float64)
    if scale is not None:
        a = np.maximum(a * np.asarray(scale, np.float64) + np.asarray(shift, np.float64), 0.0)
    y = a @ np.asarray(W, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return np.maximum(y, 0.0) if relu else y


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
def split16(a: np.ndarray):
    """fp32 -> (hi, lo) fp16 planes as fp32 arrays: hi = fp16(a), lo = fp16(a - hi)."""
    a = a.astype(np.float32)
    hi = a.astype(np.float16).astype(np.float32)
    lo = (a - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def spmm_model(L: sp.csr_matrix, x: np.ndarray) -> np.ndarray:
    """L x with fp32 products added one neighbour after the other in CSR order (the kernels' gather loops)."""
    m = L.tocsr()
    b, v, f = x.shape
    x = x.astype(np.float32)
    acc = np.zeros((b, v, f), np.float32)
    ptr, deg = m.indptr[:-1], np.diff(m.indptr)
    val = m.data.astype(np.float32)
    for j in range(int(deg.max()) if v else 0):
        rows = np.nonzero(deg > j)[0]
        e = ptr[rows] + j
        acc[:, rows, :] += val[e][None, :, None] * x[:, m.indices[e], :]
    return acc


def graph_conv_model(L, x, W, bias=None, relu=True, xin=None, up=1, drop=None) -> np.ndarray:
    """graph_conv_cheby3_ref in the fused kernel's arithmetic -> fp32.  drop: None, "lo_hi" (basis lo * bank hi left out) or
    "hi_lo" (basis hi * bank lo left out): the two-term forms a broken split product would compute."""
    if drop not in (None, "lo_hi", "hi_lo"):
        raise ValueError("drop: None, 'lo_hi' or 'hi_lo'")
    x = x.astype(np.float32)
    b, v, fin = x.shape
    basis = np.concatenate([x, spmm_model(L, x), spmm_model(cheby2(L), x)], axis=2).reshape(b * v, 3 * fin)
    ah, al = split16(basis)
    wh, wl = split16(np.asarray(W, np.float32))
    acc = np.zeros((b * v, wh.shape[0]), np.float32)
    if drop != "lo_hi":
        acc += al @ wh.T
    if drop != "hi_lo":
        acc += ah @ wl.T
    acc += ah @ wh.T
    y = acc.reshape(b, v, -1)
    if bias is not None:
        y = y + np.asarray(bias, np.float32)
    if relu:
        y = np.maximum(y, np.float32(0))
    if xin is not None:
        y = feat_interp_add_model(xin, y, 1)
    return np.repeat(y.astype(np.float32), up, axis=1)


def feat_interp_add_model(xin: np.ndarray, y: np.ndarray, up: int = 1) -> np.ndarray:
    """feat_interp_add_ref with the source index, the weights and the sum in fp32."""
    i0, i1, w1 = interp_weights(xin.shape[2], y.shape[2], np.float32)
    xi = xin.astype(np.float32)
    out = y.astype(np.float32) + ((np.float32(1) - w1) * xi[..., i0] + w1 * xi[..., i1])
    return np.repeat(out.astype(np.float32), up, axis=1)
