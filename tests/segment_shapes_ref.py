"""A numpy restatement of the contract of stocs_segment_shapes, stocs_segment_gate and stocs_segment_assign (include/stocs_hip.h): the used
pixels and their counts, the ten integer moments per label (int64: exact), centroid, covariance and axes in float64 by the kernel's own
formula and sweeps, the extents in float32 one operation at a time (taking a centroid and axes as input, so that a test can hand in the
device's own), the gate in float32, and the class stack."""
import math

import numpy as np

import segment_ref as sr

F = np.float32
EMPTY, NONFINITE = 1, 2
TOO_LARGE, TOO_SMALL, NO_SHAPE = 1, 2, 4
SWEEPS = 12
GATE_DEFAULTS = dict(slack=0.25, min_ratio=0.5, min_used=3)
SHAPE_DTYPE = np.dtype([("n_used", np.int32), ("flags", np.int32), ("centroid", np.float32, (3,)), ("eigenvalue", np.float32, (3,)), ("axis", np.float32, (3, 3)),
                        ("lo", np.float32, (3,)), ("hi", np.float32, (3,)), ("extent", np.float32, (3,)), ("reserved", np.int32, (6,))])


def used_pixels(depth_u16, labels, K, depth_scale, n_labels, max_depth):
    """step 1: the points (H, W, 3) float32, the label image with out-of-range labels set to 0, the used mask and the five counts"""
    P, valid = sr.points(depth_u16, K, depth_scale, max_depth)
    lab = np.asarray(labels, np.int32)
    oor = (lab < 0) | (lab > n_labels)
    lab = np.where(oor, 0, lab)
    labelled = lab > 0
    with np.errstate(all="ignore"):
        near = (np.abs(P) < F(16)).all(axis=-1)
    used = labelled & valid & near
    counts = dict(n_labelled=int(labelled.sum()), n_used=int(used.sum()), n_invalid=int((labelled & ~valid).sum()), n_far=int((labelled & valid & ~near).sum()),
                  n_out_of_range=int(oor.sum()))
    return P, lab, used, counts


def points_used(pos):
    """stocs_points_shape's step 1: every point is label 1, used when |x|, |y|, |z| < 16"""
    P = np.ascontiguousarray(pos, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        used = (np.abs(P) < F(16)).all(axis=-1)
    return P, np.ones(len(P), np.int32), used


def moments(P, lab, used, n_labels):
    """step 2: (n_labels, 10) int64"""
    M = np.zeros((n_labels, 10), np.int64)
    q = np.rint(P[used].astype(np.float64) * 65536.0).astype(np.int64)
    l = lab[used].astype(np.int64) - 1
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    for k, term in enumerate((np.ones_like(x), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
        np.add.at(M[:, k], l, term)
    return M


def covariance(M):
    """centroid and covariance in float64 from one label's ten moments, as the kernel forms them"""
    n = float(int(M[0])); u = 1.0 / 65536.0; uu = u * u
    c = [float(int(M[1])) / n * u, float(int(M[2])) / n * u, float(int(M[3])) / n * u]
    S = [float(int(M[4])) / n * uu - c[0] * c[0], float(int(M[5])) / n * uu - c[0] * c[1], float(int(M[6])) / n * uu - c[0] * c[2],
         float(int(M[7])) / n * uu - c[1] * c[1], float(int(M[8])) / n * uu - c[1] * c[2], float(int(M[9])) / n * uu - c[2] * c[2]]
    return c, S


def jacobi(S):
    """the library's cyclic Jacobi on Python floats (IEEE doubles): (w[3], V[3][3]), eigenvector j in column j"""
    A = [[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if A[p][q] == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
            t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0); s = t * c
            for k in range(3):
                akp, akq = A[k][p], A[k][q]; A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq
            for k in range(3):
                apk, aqk = A[p][k], A[q][k]; A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk
            for k in range(3):
                vkp, vkq = V[k][p], V[k][q]; V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq
    return [A[0][0], A[1][1], A[2][2]], V


def signed(v):
    """a unit vector whose component of largest magnitude is positive, the lowest index on equal magnitudes"""
    big = v[0]
    if abs(v[1]) > abs(big): big = v[1]
    if abs(v[2]) > abs(big): big = v[2]
    return [-x for x in v] if big < 0 else list(v)


def axes_from_moments(M):
    """step 3 for one label: (centroid float32 (3), eigenvalues float32 (3), axes float32 (3, 3) one per row, flags) and the float64 pairs"""
    c, S = covariance(M)
    w, V = jacobi(S)
    pairs = [(w[j], [V[0][j], V[1][j], V[2][j]]) for j in range(3)]
    for a, b in ((0, 1), (1, 2), (0, 1)):                       # strict: on equal values the lower column stays first
        if pairs[b][0] > pairs[a][0]:
            pairs[a], pairs[b] = pairs[b], pairs[a]
    ev, ax = [], []
    for wv, v in pairs:
        ln = math.sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]))
        ev.append(wv); ax.append(signed([x / ln for x in v]))
    good = all(math.isfinite(x) for x in c + ev + [x for a in ax for x in a])
    if not good:
        return np.array([x if math.isfinite(x) else 0.0 for x in c], F), np.zeros(3, F), np.eye(3, dtype=F), NONFINITE, (ev, ax)
    return np.array(c, np.float64).astype(F), np.array(ev, np.float64).astype(F), np.array(ax, np.float64).astype(F), 0, (ev, ax)


def eigh64(M):
    """numpy's float64 decomposition of the same covariance: eigenvalues descending, axes one per row, signed by the same rule"""
    _, S = covariance(M)
    w, v = np.linalg.eigh(np.array([[S[0], S[1], S[2]], [S[1], S[3], S[4]], [S[2], S[4], S[5]]], np.float64))
    return w[::-1].copy(), np.array([signed(list(v[:, j] / np.linalg.norm(v[:, j]))) for j in (2, 1, 0)])


def key_of(t):
    b = np.ascontiguousarray(t, F).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def unkey(k):
    k = np.asarray(k, np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(F)


def extents(P, lab, used, centroid, axis, n_labels):
    """step 4 given float32 centroids (n_labels, 3) and axes (n_labels, 3, 3): lo, hi, extent, each (n_labels, 3) float32; zero where a
    label has no used pixel"""
    p = P[used].astype(F); l = lab[used].astype(np.int64) - 1
    c = np.asarray(centroid, F)[l]; a = np.asarray(axis, F)[l]
    lo = np.full((n_labels, 3), np.iinfo(np.int32).max, np.int32); hi = np.full((n_labels, 3), np.iinfo(np.int32).min, np.int32)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - c[:, 0], p[:, 1] - c[:, 1], p[:, 2] - c[:, 2]
        for k in range(3):
            t = a[:, k, 0] * dx + (a[:, k, 1] * dy + a[:, k, 2] * dz)
            assert t.dtype == F
            key = key_of(t)
            np.minimum.at(lo[:, k], l, key); np.maximum.at(hi[:, k], l, key)
    has = np.bincount(l, minlength=n_labels) > 0
    lo_f = np.where(has[:, None], unkey(lo), F(0)).astype(F); hi_f = np.where(has[:, None], unkey(hi), F(0)).astype(F)
    return lo_f, hi_f, (hi_f - lo_f).astype(F)


def shapes_from(P, lab, used, n_labels):
    """steps 2 - 4 on the restatement's own centroid and axes: (shapes of SHAPE_DTYPE, moments)"""
    M = moments(P, lab, used, n_labels)
    s = np.zeros(n_labels, SHAPE_DTYPE)
    for l in range(n_labels):
        if M[l, 0] == 0:
            s[l]["flags"] = EMPTY
            continue
        c, ev, ax, flags, _ = axes_from_moments(M[l])
        s[l]["n_used"] = M[l, 0]; s[l]["flags"] = flags; s[l]["centroid"] = c; s[l]["eigenvalue"] = ev; s[l]["axis"] = ax
    lo, hi, ext = extents(P, lab, used, s["centroid"], s["axis"], n_labels)
    s["lo"], s["hi"], s["extent"] = lo, hi, ext
    return s, M


def segment_shapes(depth_u16, labels, K, depth_scale, n_labels, max_depth):
    P, lab, used, counts = used_pixels(depth_u16, labels, K, depth_scale, n_labels, max_depth)
    s, M = shapes_from(P, lab, used, n_labels)
    return s, M, counts


def points_shape(pos):
    P, lab, used = points_used(pos)
    s, M = shapes_from(P, lab, used, 1)
    return s[0], M[0]


def object_size(extent, diameter=None):
    """(diameter, extent[3]) float32; diameter None: the diagonal of the extents in double, cast once"""
    e = np.asarray(extent, F)
    d = F(np.sqrt(np.sum(e.astype(np.float64) ** 2))) if diameter is None else F(diameter)
    return d, e


def gate(shapes, objects, slack=0.25, min_ratio=0.5, min_used=3):
    """the reason bits (n_objects, n_labels) uint8 in float32, one operation each; objects: a list of (diameter, extent[3])"""
    out = np.zeros((len(objects), len(shapes)), np.uint8)
    for o, (diam, oext) in enumerate(objects):
        m = np.sort(np.asarray(oext, F))[::-1]
        widest = F(F(1) + F(slack)) * F(diam)
        least = F(min_ratio) * m[1]
        for l, s in enumerate(shapes):
            e1 = np.max(np.asarray(s["extent"], F))
            r = 0
            if e1 > widest: r |= TOO_LARGE
            if e1 < least: r |= TOO_SMALL
            if int(s["n_used"]) < min_used or int(s["flags"]) != 0: r |= NO_SHAPE
            out[o, l] = r
    return out


def stack(labels, n_labels, reasons):
    """the object-major uint16 class stack: image k is 10000 where the pixel's label (in 1 .. n_labels) is compatible with object k"""
    lab = np.asarray(labels, np.int32)
    lab = np.where((lab < 0) | (lab > n_labels), 0, lab)
    out = np.zeros((reasons.shape[0],) + lab.shape, np.uint16)
    for k in range(reasons.shape[0]):
        ok = np.concatenate([[False], reasons[k] == 0])
        out[k][ok[lab]] = 10000
    return out


def angle(a, b):
    """the angle between two unit vectors in float64, from the cross product (exact for small angles)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), float(a @ b)))
