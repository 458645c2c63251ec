"""numpy restatement of the mesh-component definitions of include/neusky_hip.h (nsky_cc_*): test infrastructure, no GPU, no scipy.

Two faces are connected when they share a vertex index; the root of a component is its smallest vertex index, its size its face
count; rank by size descending, then root ascending; a vertex without a face has label -1.  The roots come from min-label
propagation with pointer jumping, which shares nothing with the kernels' union-find but the definition."""
import numpy as np


def vertex_roots(V, faces):
    """root[V]: the smallest vertex index connected to each vertex through faces (a vertex without a face is its own root)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.arange(V, dtype=np.int64)
    if len(faces) == 0:
        return label
    flat = faces.ravel()
    while True:
        corner = label[faces]
        low = np.repeat(corner.min(axis=1), 3)
        new = label.copy()
        np.minimum.at(new, flat, low)            # every corner takes its face's smallest label ...
        np.minimum.at(new, corner.ravel(), low)  # ... and so does the vertex each corner's label names
        while True:                              # label[v] is a vertex connected to v: follow it down
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            # a fixed point: one label per face, hence per component; label[v] <= v and connected to v, hence the minimum
            return label
        label = new


def label_components_cpu(V, faces):
    """dict(labels [V] int32, face_labels [F] int32, roots [C] int32, face_counts [C] int64)"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    F = len(faces)
    root = vertex_roots(V, faces)
    face_root = root[faces[:, 0]] if F else np.zeros(0, np.int64)
    roots, counts = np.unique(face_root, return_counts=True)
    order = np.lexsort((roots, -counts))  # by count descending, then root ascending
    roots, counts = roots[order], counts[order]
    rank = np.full(V, -1, dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    return {"labels": rank[root].astype(np.int32), "face_labels": rank[face_root].astype(np.int32), "roots": roots.astype(np.int32),
            "face_counts": counts.astype(np.int64)}


def kept_components(face_counts, keep_largest=None, min_faces=None):
    keep = np.ones(len(face_counts), dtype=bool)
    if keep_largest is not None:
        keep &= np.arange(len(face_counts)) < keep_largest
    if min_faces is not None:
        keep &= np.asarray(face_counts) >= min_faces
    return keep


def remove_floaters_cpu(vertices, faces, keep_largest=None, min_faces=None, normals=None, colours=None):
    """dict(vertices, faces (int32), normals, colours, kept_components): the staying faces in input order, re-indexed over the
    vertices they reference (in input order); attributes are the rows of those vertices"""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(vertices)
    comps = label_components_cpu(V, faces)
    keep_c = kept_components(comps["face_counts"], keep_largest, min_faces)
    keep_f = keep_c[comps["face_labels"]] if len(faces) else np.zeros(0, bool)
    used = np.zeros(V, dtype=bool)
    used[faces[keep_f].ravel()] = True
    new_index = np.cumsum(used) - 1
    return {"vertices": vertices[used], "faces": new_index[faces[keep_f]].astype(np.int32),
            "normals": None if normals is None else normals[used], "colours": None if colours is None else colours[used],
            "kept_components": int(keep_c.sum())}
