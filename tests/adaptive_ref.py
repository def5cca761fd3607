"""numpy float32 restatement of the adaptive-sampling rule (include/sptr_hip.h, sptr_render_adaptive; DESIGN.md
§6j) — test infrastructure.  Every float operation below is one float32 numpy operation, which is correctly
rounded, in the order the header states.

run(L, ...): L[i - 1][pixel] is sample i (1-based) of the pixel, shape (max_samples, P, 3) float32 (or a function
i -> (P, 3)).  Returns (S, E, n, passes): the sums, the counts, and the passes in which some pixel was active.
"""
import numpy as np

F = np.float32


def err(S, E, n):
    """The half-buffer error of pixels with sums S, E (.., 3) and counts n (..)."""
    S, E = np.asarray(S, F), np.asarray(E, F)
    n = np.asarray(n, np.uint32)
    with np.errstate(all="ignore"):
        nf, hf = n.astype(F), (n // np.uint32(2)).astype(F)
        I, A = S / nf[..., None], E / hf[..., None]
        num = (np.abs(I[..., 0] - A[..., 0]) + np.abs(I[..., 1] - A[..., 1])) + np.abs(I[..., 2] - A[..., 2])
        s = (I[..., 0] + I[..., 1]) + I[..., 2]
        den = np.sqrt(np.where(s < F(1e-4), F(1e-4), s))  # fmax_g(s, 1e-4f): (s < 1e-4) ? 1e-4 : s, a NaN stays
        return (num / den).astype(F)


def active(S, E, n, threshold, min_samples, max_samples):
    n = np.asarray(n, np.uint32)
    with np.errstate(all="ignore"):
        converged = (n >= min_samples) & (err(S, E, n) < F(threshold))  # a NaN err: False
    return (n < max_samples) & ~converged


def take(n, min_samples, max_samples, step):
    n = np.asarray(n, np.int64)
    return np.where(n == 0, min_samples, np.minimum(step, max_samples - n)).astype(np.int64)


def run(L, threshold, min_samples, max_samples, step, state=None):
    """One call; state = (S, E, n) of an earlier call continues it (SPTR_ADAPTIVE_CONTINUE)."""
    sample = L if callable(L) else (lambda i: L[i - 1])
    P = sample(1).shape[0]
    if state is None:
        S, E, n = np.zeros((P, 3), F), np.zeros((P, 3), F), np.zeros(P, np.uint32)
    else:
        S, E, n = (np.array(a, copy=True) for a in state)
    passes = 0
    while True:
        act = active(S, E, n, threshold, min_samples, max_samples)
        if not act.any():
            break
        passes += 1
        t = np.where(act, take(n, min_samples, max_samples, step), 0)
        for s in range(int(t.max())):
            m = act & (t > s)
            i = n.astype(np.int64) + 1  # the index of each pixel's next sample
            for idx in np.unique(i[m]):
                k = m & (i == idx)
                Li = np.asarray(sample(int(idx)), F)[k]
                with np.errstate(all="ignore"):
                    S[k] = S[k] + Li
                    if idx % 2 == 0:
                        E[k] = E[k] + Li
            n[m] += np.uint32(1)
    return S, E, n, passes
