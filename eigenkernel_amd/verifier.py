"""Host-side mirror of the reference's acceptance checks (the gate the host keeps).

  eval_residual_norm   verifier.f90:75-204   ||A v_j - l_j B v_j||_2 / ||A||_F, (avg, max)
  eval_orthogonality   verifier.f90:233-330  G = V^T B V, rows/cols scaled by 1/sqrt(G_jj),
                                             diagonal zeroed, Frobenius norm
  get_ipratios         distribute_matrix.f90:18-78  sum v^4 / (sum v (S v))^2

numpy on gathered arrays (1x1 grid); the normalisations are the reference's, including the
quirk that the orthogonality check normalises by the computed G_jj instead of comparing
with 1.

The *_sygv functions carry them over to DSYGV's types 2 (A B x = l x) and 3 (B A x = l x), as
include/ek_hip.h defines them for ek_hip_check_sygv_*batched* and ek_hip_check_sygvx*; itype 1
forwards to the functions above.  A and B are symmetric by their lower triangles.
"""
import numpy as np


def eval_residual_norm(A, values, V, B=None):
    A = np.asarray(A)
    V = np.asarray(V)
    n_check = V.shape[1]
    a_norm = np.linalg.norm(A, "fro")
    R = (B @ V if B is not None else V.copy()) * (-np.asarray(values)[:n_check])
    R += A @ V
    norms = np.linalg.norm(R, axis=0)
    return a_norm, norms.sum() / a_norm / n_check, norms.max() / a_norm


def eval_orthogonality(V, B=None, index1=1, index2=None):
    V = np.asarray(V)
    index2 = V.shape[1] if index2 is None else index2
    Vs = V[:, index1 - 1:index2]
    G = Vs.T @ (B @ Vs if B is not None else Vs)
    s = 1.0 / np.sqrt(np.diag(G))
    G = G * s[:, None] * s[None, :]
    np.fill_diagonal(G, 0.0)
    return np.linalg.norm(G, "fro")


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
