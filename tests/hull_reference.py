"""An exact referee for the closest point of a small convex hull to the origin -- TEST INFRASTRUCTURE.

The device function (csrc/lscgen.hip: hull_closest_point) and the oracle (oracle/lscgen_oracle.c) are the same enumeration with the
same three constants (the degenerate-edge cut 1e-18, the degenerate-triangle cut 1e-14 g11 g22, the inside threshold |bp|^2 / 2), so
agreement between the two proves nothing about what they share.  This module shares nothing with them: no threshold, no rounding.

    closest_point(points)   points (k, 3) floats (each float is a rational number, taken as it is)

enumerates every subset of 1, 2 or 3 points, solves the subset's normal equations over the rationals and accepts the candidate c that
  * is a convex combination (all weights >= 0), and
  * carries the optimality certificate  min_i p_i . c >= c . c   (the hull lies beyond the supporting plane through c),
both tested exactly.  The closest point of a convex set is unique, so whichever subset is accepted first gives THE answer; a certificate
with c = 0 says the origin lies in the hull.  If no subset is accepted the origin is strictly inside a full-dimensional hull: the
closest point of a hull that does not contain the origin lies on its boundary, hence in a triangle of vertices (Caratheodory in the
face), hence in the relative interior of a vertex, an edge or a triangle of that triangle, whose normal equations then give it.

Arithmetic: the coordinates are scaled by a common power of two to integers, every test is a sign of an integer expression (weights
N_j / D with D > 0 the Gram determinant; certificate D sum_j N_j G_ij >= sum_jk N_j N_k G_jk); fractions.Fraction appears only in the
returned values.
"""
from collections import namedtuple
from fractions import Fraction
from itertools import combinations
import math

Closest = namedtuple("Closest", "dist point subset inside dist2 ties")
# dist: float (sqrt of the correctly rounded dist2); point: 3 Fractions; subset: the smallest accepted subset, first in enumeration
# order (the kernel's order: vertices, edges (i<j), triangles (i<j<l)); inside: the origin lies in the hull (dist == 0);
# dist2: Fraction; ties: every non-degenerate subset that yields the same point with non-negative weights (subset first)


def _integers(points):
    fr = [[Fraction(float(x)) for x in p] for p in points]
    scale = max([c.denominator for p in fr for c in p] + [1])  # denominators of floats are powers of two: the largest is the lcm
    return [[int(c * scale) for c in p] for p in fr], scale


def _weights(G, S):
    """Integer weights N (one per member of S) and D > 0 with sum N = D: the projection of the origin onto aff(S) is sum_j N_j p_Sj / D.
    None for an affinely dependent subset (a repeated point, a collinear triple): a smaller subset covers it."""
    if len(S) == 1:
        return (1,), 1
    i = S[0]
    if len(S) == 2:
        j = S[1]
        den = G[i][i] - 2 * G[i][j] + G[j][j]
        if den == 0:
            return None
        t = G[i][i] - G[i][j]
        return (den - t, t), den
    j, l = S[1], S[2]
    g11 = G[j][j] - 2 * G[i][j] + G[i][i]
    g22 = G[l][l] - 2 * G[i][l] + G[i][i]
    g12 = G[j][l] - G[i][j] - G[i][l] + G[i][i]
    r1, r2 = G[i][i] - G[i][j], G[i][i] - G[i][l]
    det = g11 * g22 - g12 * g12
    if det == 0:
        return None
    u, v = r1 * g22 - r2 * g12, r2 * g11 - r1 * g12
    return (det - u - v, u, v), det


def closest_point(points):
    P, scale = _integers(points)
    k = len(P)
    G = [[sum(a * b for a, b in zip(P[i], P[j])) for j in range(k)] for i in range(k)]
    found = None
    ties = []
    for size in (1, 2, 3):
        for S in combinations(range(k), size):
            w = _weights(G, S)
            if w is None:
                continue
            N, D = w
            if min(N) < 0:
                continue
            cc = sum(N[a] * N[b] * G[S[a]][S[b]] for a in range(size) for b in range(size))  # c . c  * D^2
            if found is not None:
                # the answer is known: a further subset ties if it reproduces the same point
                c = [Fraction(sum(N[a] * P[S[a]][x] for a in range(size)), D * scale) for x in range(3)]
                if c == found[1]:
                    ties.append(S)
                continue
            if all(D * sum(N[a] * G[i][S[a]] for a in range(size)) >= cc for i in range(k)):  # p_i . c >= c . c for every i
                c = [Fraction(sum(N[a] * P[S[a]][x] for a in range(size)), D * scale) for x in range(3)]
                found = (S, c, Fraction(cc, D * D * scale * scale))
                ties.append(S)
    if found is None:
        zero = [Fraction(0)] * 3
        return Closest(0.0, zero, (), True, Fraction(0), [])
    S, c, d2 = found
    return Closest(math.sqrt(d2), c, S, d2 == 0, d2, ties)


def certificate_holds(points, res):
    """Independent restatement of what closest_point promises, in Fractions on the points themselves: res.point is a convex
    combination of res.subset and every hull point lies beyond the supporting plane through it.  For an `inside` verdict without a
    subset (origin strictly inside) the certificate is the other way round: NO direction separates the origin, which is checked by
    showing that the origin is a strictly positive combination of four affinely independent hull points (a tetrahedron around it)."""
    fr = [[Fraction(float(x)) for x in p] for p in points]
    c = res.point
    if res.subset:
        cc = sum(x * x for x in c)
        if cc != res.dist2 or any(sum(a * b for a, b in zip(p, c)) < cc for p in fr):
            return False
        # c in conv(subset): solve for the weights again, by elimination on the subset's points
        S = res.subset
        if len(S) == 1:
            return fr[S[0]] == c
        a = fr[S[0]]
        E = [[fr[s][x] - a[x] for x in range(3)] for s in S[1:]]
        rhs = [c[x] - a[x] for x in range(3)]
        if len(S) == 2:
            ee = sum(x * x for x in E[0])
            t = sum(x * y for x, y in zip(E[0], rhs)) / ee
            return 0 <= t <= 1 and all(t * E[0][x] == rhs[x] for x in range(3))
        g11, g12, g22 = (sum(x * y for x, y in zip(E[p], E[q])) for p, q in ((0, 0), (0, 1), (1, 1)))
        b1, b2 = (sum(x * y for x, y in zip(E[p], rhs)) for p in (0, 1))
        det = g11 * g22 - g12 * g12
        u, v = (b1 * g22 - b2 * g12) / det, (b2 * g11 - b1 * g12) / det
        return u >= 0 and v >= 0 and u + v <= 1 and all(u * E[0][x] + v * E[1][x] == rhs[x] for x in range(3))
    for T in combinations(range(len(fr)), 4):
        a = fr[T[0]]
        m = [[fr[t][x] - a[x] for t in T[1:]] for x in range(3)]  # columns: edges from a
        det = (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
               + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
        if det == 0:
            continue
        # Cramer: a + m w = 0
        r = [-a[x] for x in range(3)]

        def col(j):
            mm = [row[:] for row in m]
            for x in range(3):
                mm[x][j] = r[x]
            return (mm[0][0] * (mm[1][1] * mm[2][2] - mm[1][2] * mm[2][1]) - mm[0][1] * (mm[1][0] * mm[2][2] - mm[1][2] * mm[2][0])
                    + mm[0][2] * (mm[1][0] * mm[2][1] - mm[1][1] * mm[2][0])) / det

        w = [col(0), col(1), col(2)]
        if min(w) > 0 and sum(w) < 1:
            return True
    return False


def unit_normal(res):
    """c / |c| as floats (None when inside): the exact point rounded once per component, then one division."""
    if res.inside:
        return None
    return [float(x) / res.dist for x in res.point]
