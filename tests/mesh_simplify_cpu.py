"""An independent numpy float64 restatement of the mesh-simplification definitions of include/neusky_hip.h (nsky_mesh_*) for the
tests: vertex clustering on a uniform grid with quadric-error placement (Lindstrom 2000).  numpy.linalg.eigh where the kernels run
a Jacobi iteration, dictionaries and plain loops where they sort and scan."""
import numpy as np

KEY_BITS = 21
TAU = 1e-3
BORDER = 1e-6  # a cell is borderline when an eigenvalue ratio is within BORDER (relative) of TAU or x within BORDER h of a wall


def cell_indices(vertices, lo, h):
    """[V, 3] int64: clamp(floor((p - lo) / h), 0, 2^21 - 1), float64 on the float32 coordinates"""
    p = np.asarray(vertices, np.float32).astype(np.float64)
    i = np.floor((p - np.asarray(lo, np.float64)) / np.float64(h))
    return np.clip(i, 0, 2**KEY_BITS - 1).astype(np.int64)


def cell_keys(vertices, lo, h):
    i = cell_indices(vertices, lo, h)
    return (i[:, 0] << (2 * KEY_BITS)) | (i[:, 1] << KEY_BITS) | i[:, 2]


def cluster_count(vertices, faces, lo, h):
    """faces whose three corners lie in three different cells"""
    k = cell_keys(vertices, lo, h)[np.asarray(faces, np.int64).reshape(-1, 3)]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


def face_quadrics(vertices, faces, lo):
    """[F, 10] (A00 A01 A02 A11 A12 A22 b0 b1 b2 c) of every face, coordinates relative to lo; zero rows for |m| = 0"""
    p = np.asarray(vertices, np.float32).astype(np.float64) - np.asarray(lo, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    m = np.cross(b - a, c - a)
    ln = np.sqrt((m * m).sum(1))
    ok = ln > 0
    n = np.zeros_like(m)
    n[ok] = m[ok] / ln[ok, None]
    w = np.where(ok, 0.5 * ln, 0.0)
    d = (n * a).sum(1)
    q = np.stack([w * n[:, 0] * n[:, 0], w * n[:, 0] * n[:, 1], w * n[:, 0] * n[:, 2], w * n[:, 1] * n[:, 1], w * n[:, 1] * n[:, 2],
                  w * n[:, 2] * n[:, 2], w * d * n[:, 0], w * d * n[:, 1], w * d * n[:, 2], w * d * d], 1)
    return q


def simplify_cpu(vertices, faces, lo, h, normals=None, colours=None):
    """-> dict: vertices [C, 3] float64 (not rounded to float32), faces [F', 3] int64, keys [C], cells [C, 3], quadrics [C, 10],
    quadric_abs [C, 10] (the sums of the absolute values of the terms), xbar [C, 3] (absolute coordinates), borderline [C] bool,
    counted (faces before duplicate removal), normals [C, 3] / colours [C, 3] (float, unrounded means) when given"""
    lo = np.asarray(lo, np.float64)
    h = np.float64(h)
    v32 = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    keys = cell_keys(v32, lo, h)
    ukeys, rank = np.unique(keys, return_inverse=True)
    rank = rank.reshape(-1)
    C = len(ukeys)
    cnt = np.bincount(rank, minlength=C).astype(np.float64)
    rel = v32.astype(np.float64) - lo
    xbar = np.stack([np.bincount(rank, rel[:, a], C) for a in range(3)], 1) / cnt[:, None]
    q = face_quadrics(v32, f, lo)
    Q, Qabs = np.zeros((C, 10)), np.zeros((C, 10))
    for corner in range(3):  # three records per face, also when corners share a cell
        np.add.at(Q, rank[f[:, corner]], q)
        np.add.at(Qabs, rank[f[:, corner]], np.abs(q))
    mask = 2**KEY_BITS - 1
    cells = np.stack([(ukeys >> (2 * KEY_BITS)) & mask, (ukeys >> KEY_BITS) & mask, ukeys & mask], 1)
    x = xbar.copy()
    borderline = np.zeros(C, bool)
    for c in range(C):
        A = np.array([[Q[c, 0], Q[c, 1], Q[c, 2]], [Q[c, 1], Q[c, 3], Q[c, 4]], [Q[c, 2], Q[c, 4], Q[c, 5]]])
        lam, E = np.linalg.eigh(A)
        lmax = lam.max()
        if not lmax > 0:
            continue
        ratio = lam / lmax
        borderline[c] |= bool((np.abs(ratio - TAU) <= BORDER * TAU).any())
        r = Q[c, 6:9] - A @ xbar[c]
        xs = xbar[c].copy()
        for i in range(3):
            if lam[i] > TAU * lmax:
                xs = xs + E[:, i] * (E[:, i] @ r) / lam[i]
        wall_lo, wall_hi = cells[c] * h, (cells[c] + 1) * h
        borderline[c] |= bool((np.abs(xs - wall_lo) <= BORDER * h).any() or (np.abs(xs - wall_hi) <= BORDER * h).any())
        if (xs >= wall_lo).all() and (xs <= wall_hi).all():
            x[c] = xs
    rf = rank[f]
    alive = (rf[:, 0] != rf[:, 1]) & (rf[:, 1] != rf[:, 2]) & (rf[:, 0] != rf[:, 2])
    out_faces, seen = [], set()
    for t in rf[alive]:
        s = int(np.argmin(t))
        tri = (int(t[s]), int(t[(s + 1) % 3]), int(t[(s + 2) % 3]))
        if tri not in seen:
            seen.add(tri)
            out_faces.append(tri)
    out = {"vertices": x + lo, "faces": np.array(out_faces, np.int64).reshape(-1, 3), "keys": ukeys, "cells": cells, "quadrics": Q,
           "quadric_abs": Qabs, "xbar": xbar + lo, "borderline": borderline, "counted": int(alive.sum()), "rank": rank}
    if normals is not None:
        ns = np.stack([np.bincount(rank, np.asarray(normals, np.float32)[:, a].astype(np.float64), C) for a in range(3)], 1)
        ln = np.linalg.norm(ns, axis=1)
        out["normals"] = np.where(ln[:, None] > 0, ns / np.where(ln > 0, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    if colours is not None:
        out["colours"] = np.stack([np.bincount(rank, np.asarray(colours, np.uint8)[:, a].astype(np.float64), C) for a in range(3)], 1) / cnt[:, None]
    return out


def inside_cells(vertices, cells, lo, h, slack=0.0):
    """every vertex within its cell's box [lo + i h, lo + (i + 1) h], up to `slack`"""
    v = np.asarray(vertices, np.float64)
    lo = np.asarray(lo, np.float64)
    return bool(((v >= lo + cells * h - slack) & (v <= lo + (cells + 1) * h + slack)).all())
