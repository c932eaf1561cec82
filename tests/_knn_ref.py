"""Restatements of the k nearest neighbours and of the gradient of their squared distances, for the tests of ``ga_pc_knn`` and
``ga_pc_knn_backward`` (include/ga_pointcloud.h).

``knn_f32`` follows the arithmetic contract in numpy float32 (``dist2_f32`` of tests/_pointcloud_ref.py, then a STABLE argsort: the
lowest index first among equal distances) -- the HIP kernel must reproduce it bit for bit.  ``knn_f64`` is brute force in float64,
written independently: it sorts explicit (distance, index) tuples, so on dyadic lattice clouds, where every fp32 operation is exact,
agreement of the two pins the tie rule without trusting ``argsort``.  ``knn_backward_f32`` is the contract's loop in numpy float32
(every operation rounded on its own, the sums in ascending (i, k') order); ``knn_backward_f64`` the same loop in float64, which
also returns, per component, the number of summed terms and the sum of their magnitudes for the derived error bound."""
import numpy as np

from tests._pointcloud_ref import dist2_f32


def knn_f32(query, target, K, chunk=256):
    """[Nq,3], [Nt,3] -> (dist2 [Nq,m] float32, idx [Nq,m] int64) with m = min(K, Nt), ascending, the lowest index first at ties"""
    q = np.ascontiguousarray(query, np.float32)
    t = np.ascontiguousarray(target, np.float32)
    m = min(int(K), t.shape[0])
    d2 = np.empty((q.shape[0], m), np.float32)
    idx = np.empty((q.shape[0], m), np.int64)
    for s in range(0, q.shape[0], chunk):
        d = dist2_f32(q[s:s + chunk, None, :], t[None, :, :])
        order = np.argsort(d, axis=1, kind="stable")[:, :m]
        idx[s:s + chunk] = order
        d2[s:s + chunk] = np.take_along_axis(d, order, axis=1)
    return d2, idx


def knn_f64(query, target, K):
    q = np.asarray(query, np.float64)
    t = np.asarray(target, np.float64)
    m = min(int(K), t.shape[0])
    d2 = np.empty((q.shape[0], m))
    idx = np.empty((q.shape[0], m), np.int64)
    for r in range(q.shape[0]):
        d = ((t - q[r]) ** 2).sum(1)
        pairs = sorted((float(d[j]), j) for j in range(t.shape[0]))[:m]   # lexicographic: distance, then index
        d2[r] = [p[0] for p in pairs]
        idx[r] = [p[1] for p in pairs]
    return d2, idx


def knn_padded(query, target, qlen, tlen, K):
    """A padded batch -> (dist2 [B,Nq,K] float32, idx [B,Nq,K] int64) with the zero padding of ``ga_pc_knn``"""
    B, Nq, _ = query.shape
    d2 = np.zeros((B, Nq, K), np.float32)
    idx = np.zeros((B, Nq, K), np.int64)
    for b in range(B):
        d, i = knn_f32(query[b, :qlen[b]], target[b, :tlen[b]], K)
        d2[b, :qlen[b], :d.shape[1]] = d
        idx[b, :qlen[b], :i.shape[1]] = i
    return d2, idx


def _backward(query, target, idx, grad, nq, nt, dtype, stats):
    q = np.asarray(query, dtype)
    t = np.asarray(target, dtype)
    g = np.asarray(grad, dtype)
    K = idx.shape[1]
    m = min(K, nt)
    gq = np.zeros(q.shape, dtype)
    gt = np.zeros(t.shape, dtype)
    two = dtype(2)
    if stats:
        nq_terms, nt_terms = np.zeros(q.shape, np.int64), np.zeros(t.shape, np.int64)
        aq, at = np.zeros(q.shape, np.float64), np.zeros(t.shape, np.float64)
    for i in range(nq):
        for s in range(m):
            j = int(idx[i, s])
            c = two * g[i, s]
            u = c * (q[i] - t[j])            # three components, each: one subtraction, one product
            assert u.dtype == dtype
            gq[i] = gq[i] + u
            gt[j] = gt[j] + (-u)
            if stats:
                nq_terms[i] += 1
                nt_terms[j] += 1
                aq[i] += np.abs(u)
                at[j] += np.abs(u)
    if stats:
        return gq, gt, (nq_terms, aq), (nt_terms, at)
    return gq, gt


def knn_backward_f32(query, target, idx, grad, nq=None, nt=None):
    """One cloud pair: query [Nq,3], target [Nt,3], idx [Nq,K], grad [Nq,K] -> (grad_query [Nq,3], grad_target [Nt,3]) float32.  Pairs
    (i, k') with i < nq and k' < min(K, nt) are valid, whatever the index of the others says."""
    nq = query.shape[0] if nq is None else nq
    nt = target.shape[0] if nt is None else nt
    return _backward(query, target, idx, grad, nq, nt, np.float32, False)


def knn_backward_f64(query, target, idx, grad, nq=None, nt=None):
    """-> (grad_query, grad_target, (terms, sum|u|) of the query side, (terms, sum|u|) of the target side), all float64 / int64"""
    nq = query.shape[0] if nq is None else nq
    nt = target.shape[0] if nt is None else nt
    return _backward(query, target, idx, grad, nq, nt, np.float64, True)


def grad_bound(terms, abs_sum, extra=3):
    """per component: (m + extra) * 2^-24 * sum|u|, derived, not measured: three roundings per term (2 * g, the subtraction, the
    product), each 2^-24 relative to |u|, and one per addition of the m terms, each 2^-24 relative to a partial sum <= sum|u|"""
    return (terms + extra) * 2.0 ** -24 * abs_sum
