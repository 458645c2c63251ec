"""An independent numpy restatement of the marching-cubes definitions of include/neusky_hip.h (nsky_mc_*) for the tests:
a vertex per crossing owned edge (owner flat index, then axis), faces by cell then table order, counter-clockwise seen from the
outside.  It keeps its own copy of the case table (tools/gen_mc_table.py --py prints it) and groups the cells by case, so a 128^3
grid runs in seconds.

Numbering: corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); edge e = 4 axis + u + 2 v starts at the corner with offsets
(u, v) on the two other axes (in axis order) and runs along `axis`."""
import numpy as np

# case -> triangles, 3 hex digits (edge ids) each
TRI_HEX = [
    "", "480", "095", "485895", "1a4", "1a0a80", "0951a4", "1a5a85895",
    "5b1", "4805b1", "0919b1", "4818919b1", "5b4ba4", "5b0ba0a80", "0949b4ba4", "9b8ba8",
    "286", "460620", "095286", "296956546", "1a4286", "1a0a60620", "0951a4286", "1a5a65625295",
    "5b1286", "4606205b1", "0919b1286", "4616212919b1", "2865b4ba4", "5b0ba0a60620", "0949b4ba4286", "2969b6ba6",
    "792", "480792", "025275", "752542482", "1a4792", "1a0a80792", "0252751a4", "1a5a85825275",
    "5b1792", "4805b1792", "0212717b1", "4818212717b1", "7925b4ba4", "5b0ba0a80792", "0242747b4ba4", "7b2ba2a82",
    "796986", "460670790", "085865675", "465675", "1a4796986", "1a0a60670790", "0858656751a4", "1a5a65675",
    "5b1796986", "4606707905b1", "0818616717b1", "4616717b1", "5b4ba4796986", "5b0ba0a60670790", "0878670747b4ba4", "7b6ba6",
    "6a3", "4806a3", "0956a3", "6a3485895", "134364", "130360680", "095134364", "135365685895",
    "5b16a3", "4805b16a3", "0919b16a3", "4818919b16a3", "6434535b3", "5b0b30360680", "0949b4b34364", "6838939b3",
    "2838a3", "4a0a30320", "0952838a3", "2939535434a3", "134324284", "130320", "095134324284", "135325295",
    "5b12838a3", "4a0a303205b1", "0919b12838a3", "4a2a324212919b1", "2838434535b3", "5b0b30320", "0949b4b34324284", "2939b3",
    "7926a3", "4807926a3", "0252756a3", "7525424826a3", "134364792", "130360680792", "025275134364", "135365685825275",
    "5b17926a3", "4805b17926a3", "0212717b16a3", "4818212717b16a3", "7926434535b3", "5b0b30360680792", "0242747b4b34364", "7b2b38368b82",
    "7939838a3", "4a0a30370790", "0858a5a35375", "7535434a3", "134374794984", "130370790", "085843413835375", "135375",
    "5b17939838a3", "4a0a303707905b1", "0818a7a378717b1", "4a7a374717b1", "7939838434535b3", "5b0b30370790", "0847b3", "7b3",
    "3b7", "4803b7", "0953b7", "3b7485895", "1a43b7", "1a0a803b7", "0951a43b7", "1a5a858953b7",
    "571731", "480571731", "091971731", "481891971731", "3a7a47457", "5707303a0a80", "0949747343a4", "3a7a87897",
    "2863b7", "4606203b7", "0952863b7", "2969565463b7", "1a42863b7", "1a0a606203b7", "0951a42863b7", "1a5a656252953b7",
    "571731286", "460620571731", "091971731286", "461621291971731", "2863a7a47457", "5707303a0a60620", "0949747343a4286", "29697a73a9a6",
    "3b2b92", "4803b2b92", "0252353b5", "3b2b52542482", "1a43b2b92", "1a0a803b2b92", "0252353b51a4", "1a5a858252353b5",
    "591921231", "480591921231", "021231", "481821231", "3a2a42452592", "5939235303a0a80", "0242343a4", "3a2a82",
    "3b6b96986", "4606303b0b90", "0858656353b5", "3b6b56546", "1a43b6b96986", "1a0a606303b0b90", "0858656353b51a4", "1a5a656353b5",
    "591981861631", "460630319159390", "081861631", "461631", "3a5a45356596986", "5903a6", "0838630343a4", "3a6",
    "6a7ab7", "4806a7ab7", "0956a7ab7", "4858956a7ab7", "1b4b74764", "1b0b70760680", "0951b4b74764", "1b6b76165685895",
    "5717616a1", "4805717616a1", "0919717616a1", "4818919717616a1", "574764", "570760680", "094974764", "687897",
    "2878a7ab7", "4a0ab0b70720", "0952878a7ab7", "2949542474a7ab7", "1b4b74724284", "1b0b70720", "0951b4b74724284", "1b2b72125295",
    "5717212818a1", "4a0a17157a70720", "0919717212818a1", "4a1297", "287847457", "570720", "094974724284", "297",
    "6a2ab2b92", "4806a2ab2b92", "0252656a5ab5", "6a2ab2b52542482", "1b4b94924264", "1b0b96926b60680", "02526564b41b6b5", "1b5682",
    "5919212616a1", "4805919212616a1", "0212616a1", "4818212616a1", "642452592", "596926560680", "024264", "682",
    "8a9ab9", "4a0ab0b90", "0858a5ab5", "4a5ab5", "1b4b94984", "1b0b90", "08584b41b8b5", "1b5",
    "5919818a1", "4a0a19159a90", "0818a1", "4a1", "594984", "590", "084", "",
]
TABLE = [[tuple(int(s[i + q], 16) for q in range(3)) for i in range(0, len(s), 3)] for s in TRI_HEX]
NTRI = np.array([len(t) for t in TABLE], dtype=np.int64)
OTHER = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def edge_start(e):
    """(axis, offset (dx, dy, dz) of the start corner = the owning point)"""
    a, r = divmod(e, 4)
    off = [0, 0, 0]
    off[OTHER[a][0]], off[OTHER[a][1]] = r & 1, r >> 1
    return a, tuple(off)


def edge_corners(e):
    a, off = edge_start(e)
    c0 = off[0] | (off[1] << 1) | (off[2] << 2)
    return c0, c0 | (1 << a)


def crossing_edges(case):
    return [e for e in range(12) if ((case >> edge_corners(e)[0]) & 1) != ((case >> edge_corners(e)[1]) & 1)]


def marching_cubes_cpu(volume, level=0.0, bounding_box_min=(-1.0, -1.0, -1.0), bounding_box_max=(1.0, 1.0, 1.0)):
    """volume [Nx, Ny, Nz] (float32 values) -> (vertices [V, 3] float64, faces [F, 3] int64)"""
    v = np.ascontiguousarray(np.asarray(volume, dtype=np.float32))
    nx, ny, nz = v.shape
    inside = v < np.float32(level)
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1  # vertex id of (point, axis), valid where the edge crosses
    sel = np.nonzero(flat)[0]
    p, a = sel // 3, sel % 3
    i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
    strides = np.array([ny * nz, nz, 1], dtype=np.int64)
    vf = v.reshape(-1).astype(np.float64)
    va, vb = vf[p], vf[p + strides[a]]
    t = (np.float64(np.float32(level)) - va) / (vb - va)
    lo, hi = np.asarray(bounding_box_min, np.float64), np.asarray(bounding_box_max, np.float64)
    dims = np.array([nx, ny, nz], dtype=np.float64)
    idx = np.stack([i, j, k], -1).astype(np.float64)
    idx[np.arange(len(sel)), a] += t
    verts = lo + idx / (dims - 1) * (hi - lo)

    cube = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cube |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), np.arange(nz - 1), indexing="ij")
    cell_p = (ci * ny * nz + cj * nz + ck).reshape(-1)  # the cell's minimum point (flat order of cells = flat order of points)
    cube = cube.reshape(-1)
    nt = NTRI[cube]
    first = np.cumsum(nt) - nt
    faces = np.zeros((int(nt.sum()), 3), dtype=np.int64)
    for case in np.unique(cube):
        tris = TABLE[case]
        if not tris:
            continue
        cells = np.nonzero(cube == case)[0]
        for n, tri in enumerate(tris):
            for q, e in enumerate(tri):
                ax, off = edge_start(e)
                owner = cell_p[cells] + int(off[0] * strides[0] + off[1] * strides[1] + off[2] * strides[2])
                faces[first[cells] + n, q] = vid[owner * 3 + ax]
    return verts, faces


def _edges(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)


def edge_face_counts(faces):
    """undirected edges [E, 2] (a < b) and the number of faces using each"""
    e = np.sort(_edges(faces), 1)
    return np.unique(e, axis=0, return_counts=True)


def directed_edges_unique(faces):
    """no directed edge appears twice: the faces around every edge are consistently oriented"""
    e = _edges(faces)
    return np.unique(e, axis=0).shape[0] == e.shape[0]


def euler_characteristic(n_vertices, faces):
    edges, _ = edge_face_counts(faces)
    return n_vertices - edges.shape[0] + len(faces)


def area_and_volume(verts, faces):
    """surface area and enclosed signed volume (positive for outward-facing faces)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum(), (a * np.cross(b, c)).sum() / 6.0
