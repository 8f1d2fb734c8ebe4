"""The update's last stage restated in plain Python, exact where it can be: shift of U*, gradient
step, Savitzky-Golay filter over the moving windows, clamp, publish (mppi.cpp:194-207, 420-447,
178-182; filter.cpp:19-116).  Nothing here comes from the engine, the oracle or gen_golden.py.

  * exact_weights(w, order): the filter's 2w + 1 weights as Fractions: the row of the least-squares
    pseudo-inverse that evaluates the fitted polynomial at the window's centre, from the normal
    equations (A^T A) c = e_0 solved by elimination over the rationals, weight_j = sum_p c_p x_j^p
    with x_j = j - w.  (The engine and the oracle use the Gram-polynomial recursion, gen_golden.py
    numpy's pinv.)
  * Window: MovingExtendedWindow, literally.  apply() forms sum_j weight_j uu_j exactly (Fraction)
    and rounds once to a double; that double goes back into the window, as in the reference.
  * FilterChain: everything behind the gradient.  Fed the gradient that the side under test reports,
    its U* and windows depend on the filter chain alone, not on the rollouts.

Mutants (FilterChain(mutant=...)) are the errors the smoothing tests exist to see:
  "rotate"   the weights rotated by one slot (weight_{j+1} used for slot j, cyclically)
  "split"    weight_{j+1} used for the slots j < w - 1 only: the slots sg_finish_kernel's recurrence
             handles, against the slots j >= w - 1 that it sums ahead as P_k
  "trim_gt"  trim() looks for the first time > t instead of >= t (a kept time equal to the new one
             then sits left of the window's start, and extract() reaches one slot before the window:
             that slot reads as 0 here)
and, for the case with a backwards time only:
  "clamp_failed"  the update that fails clips U*_shifted to the bounds on its way out (the reference
             leaves optimise() before the clip, so the unclipped gradient step carries over into
             an update that does not shift)
"""
from bisect import bisect_left
from fractions import Fraction

MUTANTS = ("rotate", "split", "trim_gt")


def exact_weights(w, order):
    """[2w + 1] Fractions: the Savitzky-Golay smoothing weights at the centre of 2w + 1 points for a
    polynomial of degree `order`."""
    n = order + 1
    xs = [Fraction(j - w) for j in range(2 * w + 1)]
    # normal equations: (A^T A)[p][q] = sum_j x_j^(p + q), right-hand side e_0 (the value at x = 0)
    M = [[sum(x ** (p + q) for x in xs) for q in range(n)] + [Fraction(int(p == 0))] for p in range(n)]
    for i in range(n):   # Gauss-Jordan over the rationals
        piv = next(r for r in range(i, n) if M[r][i] != 0)
        M[i], M[piv] = M[piv], M[i]
        M[i] = [v / M[i][i] for v in M[i]]
        for r in range(n):
            if r != i and M[r][i] != 0:
                f = M[r][i]
                M[r] = [a - f * b for a, b in zip(M[r], M[i])]
    c = [M[p][n] for p in range(n)]
    return [sum(c[p] * x ** p for p in range(n)) for x in xs]


class BackInTime(Exception):
    """MovingExtendedWindow::trim: "Resetting the window back in the past." """


class OutOfWindow(Exception):
    """extract() would read outside the window (undefined in the reference)."""


class Window:
    """MovingExtendedWindow(size, w) (filter.cpp:19-116)."""

    def __init__(self, size, w, trim_gt=False):
        self.w = w
        self.W = size + 2 * w + 1
        self.uu = [0.0] * self.W
        self.tt = [-1.0] * self.W
        self.start = w
        self.last_trim = -1.0
        self.trim_gt = trim_gt

    def trim(self, t):
        if t < self.last_trim:
            raise BackInTime("last reset %r, trying to reset to %r" % (self.last_trim, t))
        self.last_trim = t
        trim_idx = self.start
        for i in range(self.start):
            if (self.tt[i] > t) if self.trim_gt else (self.tt[i] >= t):
                trim_idx = i
                break
        offset = trim_idx - self.w
        assert offset >= 0   # (size_t in the reference: a negative offset would be out of its domain)
        if offset > 0:   # std::rotate left by offset, then the tail repeats the last kept element
            self.tt = self.tt[offset:] + [self.tt[-1]] * offset
            self.uu = self.uu[offset:] + [self.uu[-1]] * offset
        self.start = self.w
        self.tt[self.start] = t

    def add(self, u, t):
        assert not t < self.tt[self.start], "adding a measurement older than the new time"
        s = self.start
        self.uu[s:] = [u] * (self.W - s)   # the point, then extend()
        self.tt[s:] = [t] * (self.W - s)
        self.start += 1

    def lower_bound(self, t):
        idx = bisect_left(self.tt, t)
        assert idx < self.W
        return idx

    def apply(self, weights, t):
        """extract(t), the filter, set(t): returns the filtered value (exact sum, one rounding)."""
        idx = self.lower_bound(t)
        lo = idx - self.w
        # undefined in the reference; only the "trim_gt" mutant gets here (a time equal to the new one
        # stays left of the window's start), and for it a slot outside the window reads as 0
        if (lo < 0 or idx + self.w >= self.W) and not self.trim_gt:
            raise OutOfWindow("extract(%r) reads [%d, %d] of a window of %d" % (t, lo, idx + self.w, self.W))
        acc = Fraction(0)
        for j, wj in enumerate(weights):
            u = self.uu[lo + j] if 0 <= lo + j < self.W else 0.0
            if u != 0.0:
                acc += wj * Fraction(u)
        res = float(acc)   # int / int true division: correctly rounded
        self.uu[idx - 1] = res
        return res


def mutate_weights(weights, w, mutant):
    n = len(weights)
    if mutant == "rotate":
        return [weights[(j + 1) % n] for j in range(n)]
    if mutant == "split":
        return [weights[j + 1] if j < w - 1 else weights[j] for j in range(n)]
    return list(weights)


class FilterChain:
    """U*_shifted, U* and the C windows of one trajectory; update(t, gradient) -> U* [H][C] (lists).
    cmin / cmax None: no control bound."""

    def __init__(self, H, C, w, order, dt, gradient_step, cmin, cmax, mutant=None):
        assert mutant is None or mutant in MUTANTS or mutant == "clamp_failed"
        self.H, self.C, self.w, self.dt, self.step = H, C, w, dt, gradient_step
        self.cmin, self.cmax = cmin, cmax
        self.weights = mutate_weights(exact_weights(w, order), w, mutant)
        self.windows = [Window(H, w, trim_gt=(mutant == "trim_gt")) for _ in range(C)]
        self.clamp_failed = mutant == "clamp_failed"
        self.last_shift = 0.0
        self.U = [[0.0] * C for _ in range(H)]
        self.Us = [[0.0] * C for _ in range(H)]

    def update(self, t, gradient):
        H, C = self.H, self.C
        sb = int((t - self.last_shift) / self.dt)   # truncation (mppi.cpp:194)
        if sb > 0:
            self.last_shift = t
            kept = max(0, H - sb)
            self.Us = [list(self.U[k + sb]) if k < kept else list(self.U[H - 1]) for k in range(H)]
        for k in range(H):
            for c in range(C):
                self.Us[k][c] += float(gradient[k][c]) * self.step
        # trim raises before it changes anything, and every window holds the same last time: no
        # window is touched by a backwards time, U*_shifted keeps the gradient step, U* stays
        try:
            for win in self.windows:
                win.trim(t)
        except BackInTime:
            if self.clamp_failed:
                self._clamp()
            raise
        times = [t + float(k) * self.dt for k in range(H)]   # two roundings (mppi.cpp:430)
        for k in range(H):
            for c in range(C):
                self.windows[c].add(self.Us[k][c], times[k])
        for k in range(H):
            for c in range(C):
                self.Us[k][c] = self.windows[c].apply(self.weights, times[k])
        self._clamp()
        self.U = [list(r) for r in self.Us]
        return self.U

    def _clamp(self):
        if self.cmin is not None:
            for k in range(self.H):
                for c in range(self.C):
                    self.Us[k][c] = max(min(self.Us[k][c], float(self.cmax[c])), float(self.cmin[c]))

    def window_arrays(self):
        """(uu [C][W], tt [C][W], start [C]) as lists."""
        return ([list(w.uu) for w in self.windows], [list(w.tt) for w in self.windows], [w.start for w in self.windows])
