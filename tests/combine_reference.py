"""Float64 reference of the coherent antenna combiner, written from DESIGN.md SPEC 3.14 alone: it imports neither the product nor its
kernels.  x is always [K, n] complex (row a = antenna a of one sonde), counted from the sonde's restart.

    stats_ref / bound       M = sum x x^H per block as the 16 doubles of the read-out, and the meter's error bound on them
    weights_ref             four power iterations and the phase rule (phase="antenna0": the variant the tests show to be worse)
    apply_ref / apply_bound y = sum_a conj(w_a) x_a in float64 and the bound of the float32 fmaf chain
    combine_ref             a whole stream: per block M -> weights -> their float32 rounding -> apply"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                   # float32 unit roundoff
BLK = 256
BLOCK = 1024                     # SPEC 3.14's default block length
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def gamma(n: int, u: float = U) -> float:
    return n * u / (1.0 - n * u)


# ---------------------------------------------------------------- statistics
def stats_ref(x: np.ndarray, L: int):
    """(M [blocks, 16], A [blocks, 16]): M[:, a] = sum |x_a|^2, M[:, 4 + 2 p], M[:, 5 + 2 p] = re, im of sum x_a conj(x_c) for pair p = (a, c)
    of PAIRS; entries of antennas >= K are 0.  A = the sums of the magnitudes of each quantity's products, which bound() scales."""
    x = np.asarray(x, np.complex128)
    K, n = x.shape
    nb = n // L
    M, A = np.zeros((nb, 16)), np.zeros((nb, 16))
    xb = x[:, :nb * L].reshape(K, nb, L)
    for a in range(K):
        p = xb[a].real ** 2 + xb[a].imag ** 2
        M[:, a] = A[:, a] = p.sum(axis=1)
    for p, (a, c) in enumerate(PAIRS):
        if c >= K:
            continue
        xa, xc = xb[a], xb[c]
        cr = xa * np.conj(xc)
        M[:, 4 + 2 * p], M[:, 5 + 2 * p] = cr.real.sum(axis=1), cr.imag.sum(axis=1)
        A[:, 4 + 2 * p] = (np.abs(xa.real * xc.real) + np.abs(xa.imag * xc.imag)).sum(axis=1)
        A[:, 5 + 2 * p] = (np.abs(xa.imag * xc.real) + np.abs(xa.real * xc.imag)).sum(axis=1)
    return M, A


def bound(A: np.ndarray, L: int) -> np.ndarray:
    """|kernel - float64 sum| per block and quantity, for sums of |products| A: SPEC 3.11's bound, since the arithmetic is SPEC 3.11's
    word for word.  A product is one rounded multiplication inside one fmaf (two roundings: gamma_2 of its two terms' magnitudes); a
    sample's product then passes through 3 additions in its lane and 6 butterfly levels (gamma_9): gamma_11 of the 256-sample block's
    magnitude in all.  The block sums are exact as doubles and are added in L / 256 double additions (at most (L / 256) 2^-53 of the
    magnitudes, themselves (1 + gamma_11) larger at most); the reference's own double sum is allowed 32 * 2^-53."""
    lb = L // BLK
    return np.asarray(A) * (gamma(11) + (lb * (1.0 + gamma(11)) + 32.0) * 2.0 ** -53)


def matrix(m16: np.ndarray, K: int) -> np.ndarray:
    """the Hermitian K x K matrix of the 16 doubles"""
    M = np.zeros((K, K), np.complex128)
    for a in range(K):
        M[a, a] = m16[a]
    for p, (a, c) in enumerate(PAIRS):
        if c < K:
            M[a, c] = m16[4 + 2 * p] + 1j * m16[5 + 2 * p]
            M[c, a] = np.conj(M[a, c])
    return M


def m16_of(M: np.ndarray) -> np.ndarray:
    """the 16 doubles of a Hermitian K x K matrix"""
    K = M.shape[0]
    m = np.zeros(16)
    for a in range(K):
        m[a] = M[a, a].real
    for p, (a, c) in enumerate(PAIRS):
        if c < K:
            m[4 + 2 * p], m[5 + 2 * p] = M[a, c].real, M[a, c].imag
    return m


# ---------------------------------------------------------------- weights
def weights_ref(K: int, m16: np.ndarray, w_prev, phase: str = "previous") -> np.ndarray:
    """SPEC 3.14's rule: start from w_prev (None after a restart: the unit vector of the largest diagonal element, lowest index on
    ties), four power iterations v <- M v each normalised to unit Euclidean length (a zero norm keeps the vector), then the phase
    rule: rho = w_prev^H v, v <- v conj(rho) / |rho| if |rho| > 0.  phase="antenna0" instead turns v so that v_0 is real and positive."""
    M = matrix(np.asarray(m16, np.float64), K)
    if w_prev is None:
        v = np.zeros(K, np.complex128)
        v[int(np.argmax(np.asarray(m16[:K])))] = 1.0         # argmax: the first of equals
        prev = np.zeros(K, np.complex128)
    else:
        prev = np.asarray(w_prev, np.complex128)
        v = prev.copy()
    for _ in range(4):
        u = M @ v
        nrm = np.sqrt(np.sum(u.real ** 2 + u.imag ** 2))
        if not nrm > 0.0:
            break
        v = u / nrm
    rho = v[0] if phase == "antenna0" else np.sum(np.conj(prev) * v)
    if abs(rho) > 0.0:
        v = v * np.conj(rho) / abs(rho)
    return v


# ---------------------------------------------------------------- apply
def apply_ref(x: np.ndarray, wf: np.ndarray, L: int):
    """(y [n] complex128, T [n, 2]): y[m] = sum_a conj(wf[b, a]) x_a[m] for m in block b, in float64 with the weights as given (the
    float32 roundings that were applied); T = the sums of the magnitudes of the 2 K terms of each component, which apply_bound() scales."""
    x = np.asarray(x, np.complex128)
    K, n = x.shape
    nb = n // L
    w = np.repeat(np.asarray(wf, np.complex128)[:nb, :K], L, axis=0).T            # [K, n]
    xs = x[:, :nb * L]
    y = np.sum(np.conj(w) * xs, axis=0)
    T = np.stack([np.sum(np.abs(w.real * xs.real) + np.abs(w.imag * xs.imag), axis=0),
                  np.sum(np.abs(w.real * xs.imag) + np.abs(w.imag * xs.real), axis=0)], axis=1)
    return y, T


def apply_bound(T: np.ndarray, K: int) -> np.ndarray:
    """|kernel - float64 sum| per sample and component.  SPEC 3.14's chain adds a component's 2 K terms t_1 .. t_2K (products of two
    float32, exact in double) one after the other: t_1 is a rounded product, every further term enters through one fmaf, which rounds
    once.  t_1 therefore passes through 2 K roundings, t_j (j >= 2) through 2 K - j + 1: |err| <= gamma_2K sum |t_j| (the standard
    bound of a recursive sum whose products are exact).  sum |t_j| <= sum_a |w_a| |x_a| by Cauchy-Schwarz on each antenna's pair, so
    this is within the (2 K + 2) 2^-24 sum_a |w_a| |x_a| the order of the thing suggests.  The reference's own float64 sum of 2 K
    products is allowed 8 * 2^-53."""
    return np.asarray(T) * (gamma(2 * K) + 8.0 * 2.0 ** -53)


def apply_f32(x: np.ndarray, wf: np.ndarray, L: int) -> np.ndarray:
    """SPEC 3.14's float32 chain in numpy (an fmaf: the exact product of two float32 in double plus the addend, rounded once to
    float32): yr = wr_0 xr_0; yr = fma(wi_0, xi_0, yr); then for a = 1 ..: yr = fma(wr_a, xr_a, yr); yr = fma(wi_a, xi_a, yr); and
    yi = wr_0 xi_0; yi = fma(-wi_0, xr_0, yi); yi = fma(wr_a, xi_a, yi); yi = fma(-wi_a, xr_a, yi)."""
    K, n = x.shape
    nb = n // L
    xr, xi = x.real.astype(np.float32)[:, :nb * L], x.imag.astype(np.float32)[:, :nb * L]
    w = np.repeat(np.asarray(wf, np.complex64)[:nb, :K], L, axis=0).T
    wr, wi = w.real.astype(np.float32), w.imag.astype(np.float32)

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    yr, yi = wr[0] * xr[0], wr[0] * xi[0]
    yr, yi = fma(wi[0], xi[0], yr), fma(-wi[0], xr[0], yi)
    for a in range(1, K):
        yr = fma(wi[a], xi[a], fma(wr[a], xr[a], yr))
        yi = fma(-wi[a], xr[a], fma(wr[a], xi[a], yi))
    return yr.astype(np.float64) + 1j * yi.astype(np.float64)


# ---------------------------------------------------------------- a whole stream
def combine_ref(x: np.ndarray, L: int = BLOCK, phase: str = "previous", w_prev=None):
    """(y [n] complex128, W [blocks, K] complex128: the weights carried, M [blocks, 16]) of one sonde's stream that starts (create or
    restart) at x[:, 0], or goes on from w_prev.  The weights are applied as their float32 roundings."""
    x = np.asarray(x, np.complex128)
    K = x.shape[0]
    M, _ = stats_ref(x, L)
    W = np.zeros((len(M), K), np.complex128)
    for b in range(len(M)):
        w_prev = weights_ref(K, M[b], w_prev, phase)
        W[b] = w_prev
    wf = W.real.astype(np.float32).astype(np.float64) + 1j * W.imag.astype(np.float32).astype(np.float64)
    y, _ = apply_ref(x, wf, L)
    return y, W, M
