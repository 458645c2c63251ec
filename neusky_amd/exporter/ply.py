"""Binary little-endian PLY 1.0 writer (numpy only)."""
from __future__ import annotations

import numpy as np


def write_ply(path, mesh) -> None:
    """vertex: x y z float [, nx ny nz float] [, red green blue uchar]; face: list uchar int vertex_indices"""
    v = mesh.vertices.detach().cpu().numpy().astype("<f4", copy=False).reshape(-1, 3)
    f = mesh.faces.detach().cpu().numpy().astype("<i4", copy=False).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if mesh.normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if mesh.colours is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.empty(v.shape[0], dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if mesh.normals is not None:
        n = mesh.normals.detach().cpu().numpy().reshape(-1, 3)
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if mesh.colours is not None:
        c = mesh.colours.detach().cpu().numpy().astype(np.uint8, copy=False).reshape(-1, 3)
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(f.shape[0], dtype=[("n", "u1"), ("vertex_indices", "<i4", (3,))])
    face["n"] = 3
    face["vertex_indices"] = f
    names = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {vert.shape[0]}"]
    header += [f"property {names[t]} {n}" for n, t in fields]
    header += [f"element face {face.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
