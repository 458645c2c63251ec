#!/usr/bin/env python3
"""Generate the crack-free marching-cubes case table of neusky_amd/csrc/mesh.hip (and of tests/marching_cubes_cpu.py).

Numbering (this project's own):
  corner c in 0..7 sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from the cell's minimum point; the case is
  sum over corners of (value < level) << c.
  edge e = 4 * axis + u + 2 * v runs along `axis` from the corner whose other two offsets are (u, v), in axis order
  (x: (y, z), y: (x, z), z: (x, y)).  Its owner is that start corner, so the vertex id of edge e is the owner point's
  base id plus the rank of `axis` among the owner's crossing edges.

How a case is triangulated, so that two cells always agree on their shared face:
  1. On each cube face the crossing edges are joined by segments.  A face with two crossing edges has one segment.  An
     ambiguous face (inside corners on one diagonal, four crossing edges) separates its inside corners: each inside corner
     gets the segment between its two face edges.  The rule reads only the face's four signs, so both cells that share the
     face draw the same segments.
  2. Every crossing edge lies on two faces, so the segments close into loops.
  3. A loop is oriented so that its vector area points from the inside corners to the outside ones (increasing value).
  4. A loop is cut into triangles by diagonals none of which joins two vertices on one cube face.  Such a diagonal
     could be drawn by the neighbour across that face too, and the mesh edge would then have four faces.

Run: python tools/gen_mc_table.py [--c | --py]   (prints the C table or the compact Python strings)
"""
import sys

import numpy as np

OTHER = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_corners(e):
    a, r = divmod(e, 4)
    u, v = r & 1, r >> 1
    o1, o2 = OTHER[a]
    c0 = (u << o1) | (v << o2)
    return c0, c0 | (1 << a)


EDGES = [edge_corners(e) for e in range(12)]


def faces():
    """6 faces: (axis, side) -> (the 4 corners, the 4 edges lying in the face)"""
    out = []
    for a in range(3):
        for s in (0, 1):
            cs = [c for c in range(8) if ((c >> a) & 1) == s]
            es = [e for e in range(12) if e // 4 != a and all(((c >> a) & 1) == s for c in EDGES[e])]
            out.append((cs, es))
    return out


FACES = faces()
EDGE_FACES = [[f for f, (_, es) in enumerate(FACES) if e in es] for e in range(12)]


def share_face(e1, e2):
    return bool(set(EDGE_FACES[e1]) & set(EDGE_FACES[e2]))


def triangulations(n):
    """all triangulations of the convex n-gon 0..n-1 as lists of (i, j, k) with i < j < k"""
    def rec(i, k):
        if k - i < 2:
            return [[]]
        res = []
        for j in range(i + 1, k):
            for left in rec(i, j):
                for right in rec(j, k):
                    res.append(left + [(i, j, k)] + right)
        return res
    return rec(0, n - 1)


def case_triangles(case):
    inside = [(case >> c) & 1 for c in range(8)]
    crossing = [e for e in range(12) if inside[EDGES[e][0]] != inside[EDGES[e][1]]]
    adj = {e: [] for e in crossing}
    for cs, es in FACES:
        ce = [e for e in es if e in adj]
        if len(ce) == 2:
            segs = [tuple(ce)]
        elif len(ce) == 4:
            segs = []
            for c in cs:
                if inside[c]:
                    segs.append(tuple(e for e in es if c in EDGES[e]))
            assert len(segs) == 2
        else:
            assert not ce
            segs = []
        for a, b in segs:
            adj[a].append(b)
            adj[b].append(a)
    assert all(len(v) == 2 for v in adj.values())
    tris, seen = [], set()
    for start in crossing:
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        seen.add(start)
        while True:
            nxt = adj[cur][0] if adj[cur][0] != prev else adj[cur][1]
            if nxt == start:
                break
            loop.append(nxt)
            seen.add(nxt)
            prev, cur = cur, nxt
        mids = [(corner_pos(EDGES[e][0]) + corner_pos(EDGES[e][1])) / 2 for e in loop]
        area = sum(np.cross(mids[i], mids[(i + 1) % len(mids)]) for i in range(len(mids)))
        d = np.zeros(3)
        for e in loop:
            c0, c1 = EDGES[e]
            d += (corner_pos(c1) - corner_pos(c0)) * (1 if inside[c0] else -1)  # towards the outside corner
        dot = float(area @ d)
        assert abs(dot) > 1e-9, (case, loop)
        if dot < 0:
            loop = loop[::-1]
        best = None
        for tri in triangulations(len(loop)):
            diags = {(i, k) for t in tri for i, k in ((t[0], t[1]), (t[1], t[2]), (t[0], t[2])) if (k - i) % len(loop) not in (1, len(loop) - 1)}
            if all(not share_face(loop[i], loop[k]) for i, k in diags):
                best = tri
                break
        assert best is not None, (case, loop)
        tris += [(loop[i], loop[j], loop[k]) for i, j, k in best]
    return tris


TABLE = [case_triangles(c) for c in range(256)]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "--c"
    maxt = max(len(t) for t in TABLE)
    if mode == "--py":
        for c in range(0, 256, 8):
            print("    " + " ".join('"' + "".join("%x%x%x" % t for t in TABLE[c + i]) + '",' for i in range(8)))
        return
    print(f"// generated by tools/gen_mc_table.py: up to {maxt} triangles per case, 3 edge ids each, -1 terminated")
    print(f"__constant__ int8_t kMcTris[256][{3 * maxt + 1}] = {{")
    for c in range(256):
        row = [e for t in TABLE[c] for e in t]
        row += [-1] * (3 * maxt + 1 - len(row))
        print("    {" + ",".join(str(x) for x in row) + "},")
    print("};")
    print("__constant__ uint8_t kMcNtri[256] = {")
    for c in range(0, 256, 32):
        print("    " + ",".join(str(len(TABLE[c + i])) for i in range(32)) + ",")
    print("};")


if __name__ == "__main__":
    main()
