"""Test-side reference of SMO with one box per row: oracle/smo_oracle.py's `smo_svc` / `smo_svr` restated with a vector Cw in place
of the scalar C (0 <= alpha_i <= Cw[i], Cw[i] = C * sample_weight_i * class_weight[y_i]: libsvm's weighting), the formulas
csrc/bq_smo.hip's row-box walker implements.  Index 2 is the examined sample, index 1 its partner:

  classification  membership of row i in the free / up / low sets uses Cw[i];
                  y1 != y2: L = max(0, a2 - a1), H = min(C2, C1 + a2 - a1);  y1 == y2: L = max(0, a2 + a1 - C1), H = min(C2, a2 + a1);
                  the snap n > C - 1e-8 C ? C : (n <= 1e-8 C ? 0 : n) uses C2 for n2 and C1 for n1
  regression      kind(i) and clip(v, i) use Cw[i];  (p1, p2): L = max(0, g - C1), H = min(C2, g);  (p1, m2): L = max(0, -g),
                  H = min(C2, C1 - g);  (m1, p2): L = max(0, g), H = min(C2, C1 + g);  (m1, m2): L = max(0, -g - C1), H = min(C2, -g)

With C1 == C2 every expression is the oracle's operation for operation, so a constant Cw returns the oracle's result bit for bit
(tests/test_smo_weighted_host.py); the oracle's helpers (`_dot`, `_State`, the tie and dot modes) are imported, not copied.
"""
import numpy as np

from oracle.smo_oracle import BIG, _State, _dot


def _svc_sets(a, y, C):
    free = 0 < a < C
    up = (y == 1 and a == 0) or (y == -1 and a == C)
    low = (y == 1 and a == C) or (y == -1 and a == 0)
    return free, up, low


def smo_svc_weighted(K, y, Cw, tol=1e-3, max_outer=10 ** 9, tie='set', dot=None):
    n = len(y)
    Cw = np.asarray(Cw, dtype=float)
    s = _State()
    I0 = set()
    s.a = np.zeros(n)
    s.err = np.zeros(n)
    s.b_up, s.b_low = -1., 1.
    s.i_up = int(np.argmax(y == 1))
    s.i_low = int(np.argmax(y == -1))
    s.err[s.i_up], s.err[s.i_low] = -1., 1.
    s.steps = 0

    def thresholds_over_free():
        free = np.fromiter(I0, dtype=int, count=len(I0)) if tie == 'set' else np.flatnonzero((s.a > 0) & (s.a < Cw))
        s.b_up, s.b_low, s.i_up, s.i_low = BIG, -BIG, -1, -1
        if len(free):
            e = s.err[free]
            k = int(np.argmax(e))
            if e[k] > s.b_low:
                s.b_low, s.i_low = e[k], int(free[k])
            k = int(np.argmin(e))
            if e[k] < s.b_up:
                s.b_up, s.i_up = e[k], int(free[k])

    def step(i1, i2):
        if i1 == i2:
            return False
        a1, a2, y1, y2, E1, E2 = s.a[i1], s.a[i2], y[i1], y[i2], s.err[i1], s.err[i2]
        C1, C2 = Cw[i1], Cw[i2]
        if y1 != y2:
            L, H = max(0, a2 - a1), min(C2, C1 + a2 - a1)
        else:
            L, H = max(0, a2 + a1 - C1), min(C2, a2 + a1)
        if L == H:
            return False
        eta = K[i1, i1] + K[i2, i2] - 2 * K[i1, i2]
        if eta > 0:
            n2 = max(L, min(a2 + y2 * (E1 - E2) / eta, H))
        else:
            lo, hi = y2 * (E1 - E2) * L, y2 * (E1 - E2) * H
            n2 = L if lo > hi + 1e-12 else (H if lo < hi - 1e-12 else a2)
        if abs(n2 - a2) < 1e-12 * (n2 + a2 + 1e-12):
            return False
        n1 = a1 + y1 * y2 * (a2 - n2)
        c1, c2 = y1 * (n1 - a1), y2 * (n2 - a2)
        free = np.flatnonzero((s.a > 0) & (s.a < Cw))
        free = free[(free != i1) & (free != i2)]
        s.err[free] += c1 * K[i1, free] + c2 * K[i2, free]
        s.err[i1] += c1 * K[i1, i1] + c2 * K[i1, i2]
        s.err[i2] += c1 * K[i1, i2] + c2 * K[i2, i2]
        n2 = C2 if n2 > C2 - 1e-8 * C2 else (0. if n2 <= 1e-8 * C2 else n2)
        n1 = C1 if n1 > C1 - 1e-8 * C1 else (0. if n1 <= 1e-8 * C1 else n1)
        s.a[i1], s.a[i2] = n1, n2
        for i in (i1, i2):
            if 0 < s.a[i] < Cw[i]:
                I0.add(i)
            else:
                I0.discard(i)
        thresholds_over_free()
        for i in (i1, i2):
            free_i, up_i, low_i = _svc_sets(s.a[i], y[i], Cw[i])
            if not free_i:
                if low_i:
                    if s.err[i] > s.b_low:
                        s.b_low, s.i_low = s.err[i], i
                elif s.err[i] < s.b_up:
                    s.b_up, s.i_up = s.err[i], i
        if s.i_low == -1 or s.i_up == -1:
            raise RuntimeError('unexpected status')
        s.steps += 1
        return True

    def examine(i2):
        free, up, low = _svc_sets(s.a[i2], y[i2], Cw[i2])
        if free:
            E2 = s.err[i2]
        else:
            E2 = _dot(s.a * y, K[i2], dot, s.a != 0) - y[i2]
            s.err[i2] = E2
            if up and E2 < s.b_up:
                s.b_up, s.i_up = E2, i2
            elif low and E2 > s.b_low:
                s.b_low, s.i_low = E2, i2
        i1 = -1
        if (free or up) and s.b_low - E2 > 2 * tol:
            i1 = s.i_low
        if (free or low) and E2 - s.b_up > 2 * tol:
            i1 = s.i_up
        if i1 == -1:
            return False
        if free:
            i1 = s.i_low if s.b_low - E2 > E2 - s.b_up else s.i_up
        return step(i1, i2)

    it, changed, sweep_all = 0, 0, True
    while (changed > 0 or sweep_all) and it < max_outer:
        changed = 0
        if sweep_all:
            for i in range(n):
                changed += examine(i)
        else:
            for i in range(n):
                if 0 < s.a[i] < Cw[i]:
                    changed += examine(i)
                    if s.b_up > s.b_low - 2 * tol:
                        changed = 0
                        break
        if sweep_all:
            sweep_all = False
        elif changed == 0:
            sweep_all = True
        it += 1
    return dict(alphas=s.a, b=-(s.b_low + s.b_up) / 2, iter=it, b_up=s.b_up, b_low=s.b_low, errors=s.err,
                steps=s.steps, finished=not (changed > 0 or sweep_all))


def smo_svr_weighted(K, y, Cw, epsilon=0.1, tol=1e-3, max_outer=10 ** 9, tie='set', dot=None):
    n = len(y)
    eps = epsilon
    Cw = np.asarray(Cw, dtype=float)
    s = _State()
    I0 = set()
    s.ap, s.an, s.err = np.zeros(n), np.zeros(n), np.zeros(n)
    s.i_up = s.i_low = 0
    s.b_up, s.b_low = y[0] + eps, y[0] - eps
    s.steps = 0

    def kind(i):
        p, m, C = s.ap[i], s.an[i], Cw[i]
        if 0 < p < C or 0 < m < C:
            return 0
        if p == 0 and m == 0:
            return 1
        if p == 0 and m == C:
            return 2
        if p == C and m == 0:
            return 3
        return -1

    def clip(v, C):
        return C if v > C - 1e-10 * C else (0 if v <= 1e-10 * C else v)

    def inside():
        return ((s.ap > 0) & (s.ap < Cw)) | ((s.an > 0) & (s.an < Cw))

    def step(i1, i2):
        if i1 == i2:
            return False
        p1, m1, p2, m2 = s.ap[i1], s.an[i1], s.ap[i2], s.an[i2]
        C1, C2 = Cw[i1], Cw[i2]
        eta = max(K[i1, i1] + K[i2, i2] - 2 * K[i1, i2], 0)
        gamma = p1 - m1 + p2 - m2
        dE = s.err[i1] - s.err[i2]
        tried = [False] * 4
        changed = done = False

        def solve(L, H, base, slope_num, lin):
            if eta > 0:
                return max(L, min(base + slope_num / eta, H))
            return L if L * lin > H * lin else H

        while not done:
            if not tried[0] and (p1 > 0 or (m1 == 0 and dE > 0)) and (p2 > 0 or (m2 == 0 and dE < 0)):
                L, H = max(0, gamma - C1), min(C2, gamma)
                if L < H:
                    v2 = solve(L, H, p2, -dE, -dE)
                    v1 = p1 - (v2 - p2)
                    if abs(v1 - p1) > 1e-12 or abs(v2 - p2) > 1e-12:
                        p1, p2, changed = v1, v2, True
                else:
                    done = True
                tried[0] = True
            elif not tried[1] and (p1 > 0 or (m1 == 0 and dE > 2 * eps)) and (m2 > 0 or (p2 == 0 and dE > 2 * eps)):
                L, H = max(0, -gamma), min(C2, -gamma + C1)
                if L < H:
                    v2 = solve(L, H, m2, dE - 2 * eps, -2 * eps + dE)
                    v1 = p1 + (v2 - m2)
                    if abs(v1 - p1) > 1e-12 or abs(v2 - m2) > 1e-12:
                        p1, m2, changed = v1, v2, True
                else:
                    done = True
                tried[1] = True
            elif not tried[2] and (m1 > 0 or (p1 == 0 and dE < -2 * eps)) and (p2 > 0 or (m2 == 0 and dE < -2 * eps)):
                L, H = max(0, gamma), min(C2, C1 + gamma)
                if L < H:
                    v2 = solve(L, H, p2, -(dE + 2 * eps), -(2 * eps + dE))
                    v1 = m1 + (v2 - p2)
                    if abs(v1 - m1) > 1e-12 or abs(v2 - p2) > 1e-12:
                        m1, p2, changed = v1, v2, True
                else:
                    done = True
                tried[2] = True
            elif not tried[3] and (m1 > 0 or (p1 == 0 and dE < 0)) and (m2 > 0 or (p2 == 0 and dE > 0)):
                L, H = max(0, -gamma - C1), min(C2, -gamma)
                if L < H:
                    v2 = solve(L, H, m2, dE, dE)
                    v1 = m1 - (v2 - m2)
                    if abs(v1 - m1) > 1e-12 or abs(v2 - m2) > 1e-12:
                        m1, m2, changed = v1, v2, True
                else:
                    done = True
                tried[3] = True
            else:
                done = True
            dE += eta * ((p2 - m2) - (s.ap[i2] - s.an[i2]))
        if not changed:
            return False
        c1 = (s.ap[i1] - s.an[i1]) - (p1 - m1)
        c2 = (s.ap[i2] - s.an[i2]) - (p2 - m2)
        free = np.flatnonzero(inside())
        free = free[(free != i1) & (free != i2)]
        s.err[free] += c1 * K[i1, free] + c2 * K[i2, free]
        s.err[i1] += c1 * K[i1, i1] + c2 * K[i1, i2]
        s.err[i2] += c1 * K[i1, i2] + c2 * K[i2, i2]
        s.ap[i1], s.ap[i2], s.an[i1], s.an[i2] = clip(p1, C1), clip(p2, C2), clip(m1, C1), clip(m2, C2)
        for i in (i1, i2):
            if kind(i) == 0:
                I0.add(i)
            else:
                I0.discard(i)
        s.b_up, s.b_low, s.i_up, s.i_low = BIG, -BIG, -1, -1
        scan = list(I0) if tie == 'set' else np.flatnonzero(inside())
        for i in scan:
            pin, nin, e = 0 < s.ap[i] < Cw[i], 0 < s.an[i] < Cw[i], s.err[i]
            if pin and e - eps > s.b_low:
                s.b_low, s.i_low = e - eps, int(i)
            elif nin and e + eps > s.b_low:
                s.b_low, s.i_low = e + eps, int(i)
            if pin and e - eps < s.b_up:
                s.b_up, s.i_up = e - eps, int(i)
            elif nin and e + eps < s.b_up:
                s.b_up, s.i_up = e + eps, int(i)
        for i in (i1, i2):
            k = kind(i)
            if k != 0:
                if k == 2 and s.err[i] + eps > s.b_low:
                    s.b_low, s.i_low = s.err[i] + eps, i
                elif k == 1 and s.err[i] - eps > s.b_low:
                    s.b_low, s.i_low = s.err[i] - eps, i
                if k == 3 and s.err[i] - eps < s.b_up:
                    s.b_up, s.i_up = s.err[i] - eps, i
                elif k == 1 and s.err[i] + eps < s.b_up:
                    s.b_up, s.i_up = s.err[i] + eps, i
        if s.i_low == -1 or s.i_up == -1:
            raise RuntimeError('unexpected status')
        s.steps += 1
        return True

    def pick(E_low_side, E_up_side):
        if s.b_low - E_low_side > 2 * tol:
            return s.i_up if E_low_side - s.b_up > s.b_low - E_low_side else s.i_low
        if E_up_side - s.b_up > 2 * tol:
            return s.i_low if s.b_low - E_up_side > E_up_side - s.b_up else s.i_up
        return -1

    def examine(i2):
        p2, m2, C2 = s.ap[i2], s.an[i2], Cw[i2]
        k = kind(i2)
        if k == 0:
            E2 = s.err[i2]
        else:
            E2 = y[i2] - _dot(s.ap - s.an, K[i2], dot, (s.ap != 0) | (s.an != 0))
            s.err[i2] = E2
            if k == 1:
                if E2 + eps < s.b_up:
                    s.b_up, s.i_up = E2 + eps, i2
                elif E2 - eps > s.b_low:
                    s.b_low, s.i_low = E2 - eps, i2
            elif k == 2 and E2 + eps > s.b_low:
                s.b_low, s.i_low = E2 + eps, i2
            elif k == 3 and E2 - eps < s.b_up:
                s.b_up, s.i_up = E2 - eps, i2
        i1 = -1
        if k == 0:
            if 0 < p2 < C2:
                i1 = pick(E2 - eps, E2 - eps)
            elif 0 < m2 < C2:
                i1 = pick(E2 + eps, E2 + eps)
        elif k == 1:
            i1 = pick(E2 + eps, E2 - eps)
        elif k == 2:
            if (E2 + eps) - s.b_up > 2 * tol:
                i1 = s.i_up
        elif k == 3:
            if s.b_low - (E2 - eps) > 2 * tol:
                i1 = s.i_low
        else:
            raise RuntimeError('the index could not be found')
        if i1 == -1:
            return False
        return step(i1, i2)

    it, changed, sweep_all = 0, 0, True
    while (changed > 0 or sweep_all) and it < max_outer:
        changed = 0
        if sweep_all:
            for i in range(n):
                changed += examine(i)
        else:
            for i in range(n):
                if 0 < s.ap[i] < Cw[i] or 0 < s.an[i] < Cw[i]:
                    changed += examine(i)
                    if s.b_up > s.b_low - 2 * tol:
                        changed = 0
                        break
        if sweep_all:
            sweep_all = False
        elif changed == 0:
            sweep_all = True
        it += 1
    return dict(alphas_p=s.ap, alphas_n=s.an, b=(s.b_low + s.b_up) / 2, iter=it, b_up=s.b_up, b_low=s.b_low,
                errors=s.err, steps=s.steps, finished=not (changed > 0 or sweep_all))
