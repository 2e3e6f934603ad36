"""Host-side mirror of the reference's acceptance checks (the gate the host keeps).

  eval_residual_norm   verifier.f90:75-204   ||A v_j - l_j B v_j||_2 / ||A||_F, (avg, max)
  eval_orthogonality   verifier.f90:233-330  G = V^T B V, rows/cols scaled by 1/sqrt(G_jj),
                                             diagonal zeroed, Frobenius norm
  get_ipratios         distribute_matrix.f90:18-78  sum v^4 / (sum v (S v))^2

numpy on gathered arrays (1x1 grid); the normalisations are the reference's, including the
quirk that the orthogonality check normalises by the computed G_jj instead of comparing
with 1.  Products and sums of squares are float64, as the kernels form them; the square roots, reciprocals and
divisions that follow them in eval_residual_norm and eval_orthogonality run in long double and are rounded once, so that
on data whose sums are exact the mirror returns the correctly rounded value (tests/test_verify_cases_host.py).

The *_sygv functions carry them over to DSYGV's types 2 (A B x = l x) and 3 (B A x = l x), as
include/ek_hip.h defines them for ek_hip_check_sygv_*batched* and ek_hip_check_sygvx*; itype 1
forwards to the functions above.  A and B are symmetric by their lower triangles.
"""
import numpy as np


_L = np.longdouble      # the last square roots and divisions: one rounding to float64 at the very end


def eval_residual_norm(A, values, V, B=None):
    A = np.asarray(A)
    V = np.asarray(V)
    n_check = V.shape[1]
    R = (B @ V if B is not None else V.copy()) * (-np.asarray(values)[:n_check])
    R += A @ V
    # float64 products and sums of squares, as the kernels form them; what follows them in long double, so that on
    # exact data the result is the correctly rounded value
    a_norm = np.sqrt(_L((A * A).sum()))
    norms = np.sqrt((R * R).sum(axis=0).astype(_L))
    return np.float64(a_norm), np.float64(norms.sum() / a_norm / n_check), np.float64(norms.max() / a_norm)


def _scaled_offdiagonal_norm(G):
    """|| D^-1/2 G D^-1/2 with zero diagonal ||_F, D = diag(G): the scaling and the sum in long double, by column blocks"""
    d = np.diag(G).astype(_L)
    s = 1 / np.sqrt(d)
    total = _L(0)
    for c in range(0, G.shape[1], 256):
        blk = G[:, c:c + 256].astype(_L) * s[:, None] * s[None, c:c + 256]
        k = np.arange(c, c + blk.shape[1])
        blk[k, k - c] = 0
        total += (blk * blk).sum()
    return np.float64(np.sqrt(total))


def eval_orthogonality(V, B=None, index1=1, index2=None):
    V = np.asarray(V)
    index2 = V.shape[1] if index2 is None else index2
    Vs = V[:, index1 - 1:index2]
    G = Vs.T @ (B @ Vs if B is not None else Vs)
    return _scaled_offdiagonal_norm(G)


def get_ipratios(V, S=None):
    V = np.asarray(V)
    SV = S @ V if S is not None else V
    p4 = (V ** 4).sum(axis=0)
    p2 = (V * SV).sum(axis=0)
    return p4 / p2 ** 2


def _sym_lower(M):
    M = np.asarray(M, dtype=np.float64)
    return np.tril(M) + np.tril(M, -1).T


def _metric_sygv(itype, V, B):
    """The metric G of the type: Z^T B Z (types 1, 2) or (L^-1 Z)^T (L^-1 Z) with B = L L^T (type 3; NaN if B is not
    SPD)."""
    if itype not in (1, 2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    V = np.asarray(V, dtype=np.float64)
    B = _sym_lower(B)
    if itype != 3:
        return V.T @ (B @ V)
    L = np.tril(B)                                  # B = L L^T, right-looking with divisions, as the check's own factor
    for k in range(L.shape[0]):
        d = L[k, k]
        if not (d > 0.0 and np.isfinite(d)):
            return np.full((V.shape[1], V.shape[1]), np.nan)
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    W = V.copy()                                    # W = L^-1 V by forward substitution, a column of L a step
    for k in range(L.shape[0]):
        W[k] /= L[k, k]
        W[k + 1:] -= np.outer(L[k + 1:, k], W[k])
    return W.T @ W


def eval_residual_norm_sygv(itype, A, B, values, V):
    """(norm, res_ave, res_max): norm = ||A||_F (type 1) or ||A||_F ||B||_F; rho_j = ||r_j|| / norm for type 1, else
    ||A (B v_j) - l_j v_j|| (type 2) or ||B (A v_j) - l_j v_j|| (type 3) over norm ||v_j||."""
    if itype == 1:
        return eval_residual_norm(_sym_lower(A), values, V, _sym_lower(B))
    if itype not in (2, 3):
        raise ValueError("itype must be 1, 2 or 3")
    A, B = _sym_lower(A), _sym_lower(B)
    V = np.asarray(V, dtype=np.float64)
    n_check = V.shape[1]
    norm = np.linalg.norm(A, "fro") * np.linalg.norm(B, "fro")
    R = (A @ (B @ V) if itype == 2 else B @ (A @ V)) - V * np.asarray(values)[:n_check]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.linalg.norm(R, axis=0) / (norm * np.linalg.norm(V, axis=0))
    return norm, rho.sum() / n_check, rho.max()


def eval_orthogonality_sygv(itype, V, B):
    if itype == 1:
        return eval_orthogonality(V, _sym_lower(B))
    G = _metric_sygv(itype, V, B)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = 1.0 / np.sqrt(np.diag(G))
        G = G * s[:, None] * s[None, :]
    np.fill_diagonal(G, 0.0)
    return np.linalg.norm(G, "fro")


def get_ipratios_sygv(itype, V, B):
    if itype == 1:
        return get_ipratios(V, _sym_lower(B))
    V = np.asarray(V, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        V2 = V * V                                  # z^4 as the square of the square, as the kernels form it
        return (V2 * V2).sum(axis=0) / np.diag(_metric_sygv(itype, V, B)) ** 2
