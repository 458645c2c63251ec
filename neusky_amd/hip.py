"""ctypes binding of libneusky_hip.so (the C ABI declared in include/neusky_hip.h).

Fails loudly when the shared library is missing: the product path has no fallback.  Tensors are
passed as raw device pointers (`tensor.data_ptr()`), the stream as torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libneusky_hip.so")


class NeuSkyHipError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
        "neusky_amd has no CPU/PyTorch fallback."
    )
_lib = C.CDLL(LIB_PATH)

# ---- epilogues (keep in sync with include/neusky_hip.h)
EPI_NONE, EPI_RELU, EPI_LEAKY, EPI_SIGMOID, EPI_SOFTPLUS, EPI_FILM, EPI_MUL_AUX = 0, 1, 2, 3, 4, 5, 6
EPI_BWD_RELU, EPI_BWD_LEAKY, EPI_BWD_FILM, EPI_EXP = 7, 8, 9, 10
PREC_F32, PREC_BF16X2, PREC_BF16X3, PREC_F16X2 = 0, 2, 3, 4


class GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("ldb", C.c_int32), ("ldc", C.c_int32),
        ("a_kcontig", C.c_int32), ("b_kcontig", C.c_int32),
        ("bias", C.c_void_p),
        ("epi", C.c_int32), ("p0", C.c_float), ("p1", C.c_float),
        ("aux0", C.c_void_p), ("ldaux0", C.c_int32),
        ("aux1", C.c_void_p), ("ldaux1", C.c_int32),
        ("aux2", C.c_void_p), ("ldaux2", C.c_int32),
        ("out1", C.c_void_p), ("ldout1", C.c_int32),
        ("out2", C.c_void_p), ("ldout2", C.c_int32),
        ("row_mod", C.c_int32), ("k_splits", C.c_int32), ("beta", C.c_float), ("a_rowsum", C.c_void_p), ("precision", C.c_int32),
        ("rowsum_k_limit", C.c_int32),
        ("a_native_nt", C.c_int32), ("b_native_nt", C.c_int32), ("a_scale_max", C.c_void_p),
    ]


_lib.nsky_last_error.restype = C.c_char_p
_lib.nsky_abi_version.restype = C.c_int
ABI_VERSION = 18  # the ctypes structures below mirror this version of include/neusky_hip.h
if _lib.nsky_abi_version() != ABI_VERSION:
    raise NeuSkyHipError(f"libneusky_hip.so has ABI version {_lib.nsky_abi_version()}, this package binds version {ABI_VERSION}: rebuild (build.sh)")


def _sig(name, *argtypes):
    fn = getattr(_lib, name)
    fn.restype = C.c_int
    fn.argtypes = list(argtypes)
    return fn


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NeuSkyHipError(f"{what} failed ({rc}): {_lib.nsky_last_error().decode()}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """device address of a tensor handed to the C ABI.  A host tensor is an error: there is no CPU path behind these entry points."""
    if t is None:
        return None
    if not t.is_cuda:
        raise NeuSkyHipError(f"host tensor {tuple(t.shape)} handed to a HIP entry point: the product path runs on the device only "
                             "(the CPU restatement is oracle/, test infrastructure)")
    return t.data_ptr()


def ld(t):
    """leading dimension (elements) of a 2-D row-major view whose rows are contiguous"""
    if t is None:
        return 0
    st = t.stride()
    if len(st) != 2 or st[1] != 1:
        raise ValueError(f"expected a 2-D view with contiguous rows, got shape {tuple(t.shape)} stride {st}")
    return st[0]


_gemm = _sig("nsky_gemm_f32", C.POINTER(GemmDesc), C.c_void_p)
_colsum = _sig("nsky_colsum_f32", C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)


def gemm(A, B, Cout, M, N, K, *, a_kcontig=True, b_kcontig=True, bias=None, epi=EPI_NONE, p0=0.0, p1=0.0,
         aux0=None, aux1=None, aux2=None, out1=None, out2=None, row_mod=0, k_splits=0, beta=0.0, a_rowsum=None, precision=0,
         rowsum_k_limit=0, a_native_nt=0, b_native_nt=0, a_scale_max=None):
    """C[M,N] = epi(sum_k A(m,k) B(n,k) + bias).  A/B/C are 2-D row-major views (rows contiguous); a_native_nt / b_native_nt:
    that operand is a tile-native matrix (include/neusky_hip.h) with this many 32-feature tiles per row."""
    d = GemmDesc(
        A=ptr(A), B=ptr(B), C=ptr(Cout), M=M, N=N, K=K, lda=ld(A), ldb=ld(B), ldc=ld(Cout),
        a_kcontig=int(a_kcontig), b_kcontig=int(b_kcontig), bias=ptr(bias), epi=epi, p0=p0, p1=p1,
        aux0=ptr(aux0), ldaux0=ld(aux0), aux1=ptr(aux1), ldaux1=ld(aux1), aux2=ptr(aux2), ldaux2=ld(aux2),
        out1=ptr(out1), ldout1=ld(out1), out2=ptr(out2), ldout2=ld(out2), row_mod=row_mod, k_splits=k_splits, beta=beta,
        a_rowsum=ptr(a_rowsum), precision=precision, rowsum_k_limit=rowsum_k_limit,
        a_native_nt=a_native_nt, b_native_nt=b_native_nt, a_scale_max=ptr(a_scale_max),
    )
    check(_gemm(C.byref(d), stream_ptr()), "nsky_gemm_f32")
    return Cout


_split_planes = _sig("nsky_split_planes", C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                     C.c_int32, C.c_int32, C.c_void_p)
_gemm_planes = _sig("nsky_gemm_f32_planes", C.POINTER(GemmDesc), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)


def split_planes(W, n_rows, n_k, transpose, precision):
    """two 16-bit planes [2, rows_pad, ldp] (int16 storage) of a weight matrix for gemm_planes; see include/neusky_hip.h"""
    rows_pad, ldp = (n_rows + 255) // 256 * 256, (n_k + 31) // 32 * 32
    planes = torch.empty(2, rows_pad, ldp, dtype=torch.int16, device=W.device)
    check(_split_planes(ptr(W), n_rows, n_k, ld(W), int(transpose), precision, planes[0].data_ptr(), planes[1].data_ptr(),
                        rows_pad, ldp, stream_ptr()), "nsky_split_planes")
    return planes


def gemm_planes(A, planes, Cout, M, N, K, *, precision, bias=None, epi=EPI_NONE, p0=0.0, p1=0.0, aux0=None, aux1=None, aux2=None,
                out1=None, out2=None, row_mod=0, beta=0.0):
    """C[M,N] = epi(sum_k A(m,k) B(n,k) + bias) with B given as the planes of split_planes (LDS-DMA kernel)"""
    d = GemmDesc(
        A=ptr(A), B=None, C=ptr(Cout), M=M, N=N, K=K, lda=ld(A), ldb=0, ldc=ld(Cout), a_kcontig=1, b_kcontig=1, bias=ptr(bias),
        epi=epi, p0=p0, p1=p1, aux0=ptr(aux0), ldaux0=ld(aux0), aux1=ptr(aux1), ldaux1=ld(aux1), aux2=ptr(aux2), ldaux2=ld(aux2),
        out1=ptr(out1), ldout1=ld(out1), out2=ptr(out2), ldout2=ld(out2), row_mod=row_mod, k_splits=0, beta=beta,
        a_rowsum=None, precision=precision,
    )
    check(_gemm_planes(C.byref(d), planes[0].data_ptr(), planes[1].data_ptr(), planes.shape[2], stream_ptr()), "nsky_gemm_f32_planes")
    return Cout


_wcolsum = _sig("nsky_weighted_colsum_f32", C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)


def weighted_colsum(X, M, N, w, w_stride, out):
    """out[c] += sum_r w[r * w_stride] X[r, c]"""
    check(_wcolsum(ptr(X), M, N, ld(X), ptr(w), w_stride, ptr(out), stream_ptr()), "nsky_weighted_colsum_f32")
    return out


def colsum(X, M, N, out):
    check(_colsum(ptr(X), M, N, ld(X), ptr(out), stream_ptr()), "nsky_colsum_f32")
    return out


def abi_version() -> int:
    return _lib.nsky_abi_version()


# ------------------------------------------------------------------------------------------ hash grid
class HashGridDesc(C.Structure):
    _fields_ = [
        ("table", C.c_void_p), ("n_levels", C.c_int32), ("smoothstep", C.c_int32),
        ("scale", C.c_float * 16), ("resolution", C.c_int32 * 16), ("offset", C.c_uint32 * 17),
    ]


MODE_RAW, MODE_CONTRACT_LINF, MODE_CONTRACT_L2 = 0, 1, 2

_encode_fwd = _sig("nsky_encode_fwd", C.POINTER(HashGridDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                   C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_encode_bwd = _sig("nsky_encode_bwd", C.POINTER(HashGridDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                   C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_encode_fwd_dir = _sig("nsky_encode_fwd_dir", C.POINTER(HashGridDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_encode_bwd_dir = _sig("nsky_encode_bwd_dir", C.POINTER(HashGridDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                       C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_encode_bwd_ws = _lib.nsky_encode_bwd_workspace_bytes
_encode_bwd_ws.restype = C.c_int64
_encode_bwd_ws.argtypes = [C.POINTER(HashGridDesc), C.c_int32, C.c_int32]
_hash_indices = _sig("nsky_hash_indices", C.POINTER(HashGridDesc), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)


def grid_desc(geom, table) -> HashGridDesc:
    """geom: neusky_amd.encoding.HashGridGeometry; table: [n_params, 2] float32 device tensor."""
    assert table.is_cuda and table.dtype == torch.float32 and table.is_contiguous() and table.shape == (geom.n_params, 2)
    d = HashGridDesc(table=table.data_ptr(), n_levels=geom.n_levels, smoothstep=int(geom.smoothstep))
    for i in range(geom.n_levels):
        d.scale[i] = geom.scales[i]
        d.resolution[i] = geom.resolutions[i]
    for i in range(geom.n_levels + 1):
        d.offset[i] = geom.offsets[i]
    return d


def encode_fwd(geom, table, x, mode, include_x, pe_freqs, pe_max_exp, Y, T=None):
    P = x.shape[0]
    assert x.shape == (P, 3) and x.is_contiguous() and Y.shape[0] == P
    if T is not None:
        assert T.shape == (3, P, Y.shape[1]) and T.is_contiguous() and Y.is_contiguous()
    check(_encode_fwd(C.byref(grid_desc(geom, table)), ptr(x), P, mode, int(include_x), pe_freqs, pe_max_exp, ptr(Y), ld(Y),
                      ptr(T), stream_ptr()), "nsky_encode_fwd")
    return Y


def encode_bwd(geom, table, x, mode, include_x, pe_freqs, pe_max_exp, dY, dT, dtable, dx=None, workspace="auto"):
    """workspace: "auto" allocates the scratch nsky_encode_bwd_workspace_bytes asks for (large batches: the fine levels' gradient
    is then accumulated by chunk-owning workgroups in LDS); None: the direct global-atomic scatter whatever the batch"""
    P = x.shape[0]
    if dT is not None:
        assert dT.shape == (3, P, dY.shape[1]) and dT.is_contiguous() and dY.is_contiguous()
    assert dtable is None or (dtable.shape == table.shape and dtable.is_contiguous())
    desc = grid_desc(geom, table)
    if isinstance(workspace, str):
        nbytes = _encode_bwd_ws(C.byref(desc), P, int(dT is not None)) if dtable is not None else 0
        workspace = torch.empty(nbytes // 4, dtype=torch.int32, device=x.device) if nbytes > 0 else None
    check(_encode_bwd(C.byref(desc), ptr(x), P, mode, int(include_x), pe_freqs, pe_max_exp, ptr(dY), ld(dY),
                      ptr(dT), ptr(dtable), ptr(dx), ptr(workspace), stream_ptr()), "nsky_encode_bwd")


def _check_dirs(dirs, P):
    """directions of the directional encode: [R, 3] with P = R * spr (point p takes direction p // spr) -> spr"""
    R = dirs.shape[0]
    assert dirs.shape == (R, 3) and dirs.is_contiguous() and dirs.dtype == torch.float32 and R >= 1 and P % R == 0, (dirs.shape, P)
    return P // R


def encode_fwd_dir(geom, table, x, mode, include_x, pe_freqs, pe_max_exp, dirs, Y, Td):
    """Y [P, ld] and ONE tangent row-set Td [P, ld] = sum_a d_a T_a; dirs [R, 3], P = R * spr"""
    P = x.shape[0]
    assert x.shape == (P, 3) and x.is_contiguous() and Y.shape[0] == P and Td.shape == Y.shape and Y.is_contiguous() and Td.is_contiguous()
    spr = _check_dirs(dirs, P)
    check(_encode_fwd_dir(C.byref(grid_desc(geom, table)), ptr(x), P, mode, int(include_x), pe_freqs, pe_max_exp, ptr(dirs), spr, ptr(Y), ld(Y),
                          ptr(Td), stream_ptr()), "nsky_encode_fwd_dir")
    return Y


def encode_bwd_dir(geom, table, x, mode, include_x, pe_freqs, pe_max_exp, dirs, dY, dTd, dtable, workspace="auto"):
    """the table gradient of encode_fwd_dir: what encode_bwd adds for dT_a = d_a dTd"""
    P = x.shape[0]
    assert dTd.shape == dY.shape and dY.shape[0] == P and dTd.is_contiguous() and dY.is_contiguous() and ld(dTd) == ld(dY)
    assert dtable.shape == table.shape and dtable.is_contiguous()
    spr = _check_dirs(dirs, P)
    desc = grid_desc(geom, table)
    if isinstance(workspace, str):
        nbytes = _encode_bwd_ws(C.byref(desc), P, 1)
        workspace = torch.empty(nbytes // 4, dtype=torch.int32, device=x.device) if nbytes > 0 else None
    check(_encode_bwd_dir(C.byref(desc), ptr(x), P, mode, int(include_x), pe_freqs, pe_max_exp, ptr(dirs), spr, ptr(dY), ld(dY), ptr(dTd),
                          ptr(dtable), ptr(workspace), stream_ptr()), "nsky_encode_bwd_dir")


def hash_indices(geom, table, x, mode):
    P = x.shape[0]
    out = torch.empty(P, geom.n_levels, 8, dtype=torch.int32, device=x.device)
    check(_hash_indices(C.byref(grid_desc(geom, table)), ptr(x), P, mode, ptr(out), stream_ptr()), "nsky_hash_indices")
    return out


# ------------------------------------------------------------------------------------------ sample generators
_ddf_vmf_samples = _sig("nsky_ddf_vmf_samples", C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p)


def ddf_vmf_samples(n_positions, n_directions, kappa, radius, upper_hemisphere, seed, counter, origins, directions):
    """counter: int64 device tensor [1] (advanced by one); origins / directions: [n_positions * n_directions, 3] float32"""
    n = n_positions * n_directions
    assert counter.dtype == torch.int64 and counter.numel() == 1 and counter.is_cuda
    assert origins.shape == (n, 3) and directions.shape == (n, 3) and origins.is_contiguous() and directions.is_contiguous()
    check(_ddf_vmf_samples(n_positions, n_directions, float(kappa), float(radius), int(upper_hemisphere), int(seed) & (2**64 - 1),
                           ptr(counter), ptr(origins), ptr(directions), stream_ptr()), "nsky_ddf_vmf_samples")


_illum_dirs = _sig("nsky_illumination_directions", C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p)


def illumination_directions(base, rotation, seed, counter, dirs, sel, rot_out=None):
    """base [D,3] -> dirs [D,3] = base R^T, sel [D/2] int32 (ascending indices of the upper half); R = rotation [3,3] or drawn from
    (seed, counter) when rotation is None (counter: int64 device tensor [1], advanced by one)"""
    D = base.shape[0]
    assert base.is_contiguous() and dirs.is_contiguous() and dirs.shape == (D, 3) and sel.dtype == torch.int32 and sel.numel() == D // 2
    assert rotation is None or (rotation.is_contiguous() and rotation.shape == (3, 3) and rotation.dtype == torch.float32)
    assert rotation is not None or (counter.dtype == torch.int64 and counter.numel() == 1)
    check(_illum_dirs(ptr(base), D, ptr(rotation), int(seed) & (2**64 - 1), ptr(counter), ptr(dirs), ptr(sel), ptr(rot_out), stream_ptr()),
          "nsky_illumination_directions")


_fit_rows_fwd = _sig("nsky_ddf_fit_rows_fwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                     C.c_void_p, C.c_void_p, C.c_void_p)
_fit_rows_bwd = _sig("nsky_ddf_fit_rows_bwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                     C.c_void_p)


def ddf_fit_rows_fwd(positions, directions, term_dist, mv_points_in, seed, counter, sky_o, sky_d, radius, want_mv, weight_exp,
                     weight_include_z, q_pos, xrow, mv_points_out, sky_gt, distance_weight):
    """rows of the DDF-fit evaluations (fit rays | multi-view | sky) into q_pos [E,3] / xrow [E,ld]; see include/neusky_hip.h"""
    N, Ns = positions.shape[0], (0 if sky_o is None else sky_o.shape[0])
    E = N + (N if want_mv else 0) + Ns
    assert q_pos.shape[0] == E and xrow.shape[0] == E and q_pos.stride() == (3, 1)
    for t in (positions, directions, term_dist, mv_points_in, sky_o, sky_d, mv_points_out, sky_gt, distance_weight):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
    check(_fit_rows_fwd(ptr(positions), ptr(directions), ptr(term_dist), N, ptr(mv_points_in), int(seed) & (2**64 - 1), ptr(counter),
                        ptr(sky_o), ptr(sky_d), Ns, float(radius), int(want_mv), float(weight_exp), int(weight_include_z), ptr(q_pos),
                        ptr(xrow), ld(xrow), ptr(mv_points_out), ptr(sky_gt), ptr(distance_weight), stream_ptr()), "nsky_ddf_fit_rows_fwd")


def ddf_fit_rows_bwd(positions, directions, term_dist, mv_points, d_xrow_mv, d_term_dist):
    N = positions.shape[0]
    assert d_xrow_mv.shape[0] == N and d_term_dist.numel() == N
    check(_fit_rows_bwd(ptr(positions), ptr(directions), ptr(term_dist), ptr(mv_points), N, ptr(d_xrow_mv), ld(d_xrow_mv), ptr(d_term_dist),
                        stream_ptr()), "nsky_ddf_fit_rows_bwd")


_reni_in_fwd = _sig("nsky_reni_grid_inputs_fwd", C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                    C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p)
_reni_in_bwd = _sig("nsky_reni_grid_inputs_bwd", C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                    C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)


def reni_grid_inputs_fwd(latents, directions, ray_dirs, ray_latent, cond, xrow):
    U, L, _ = latents.shape
    D = directions.shape[0]
    R = 0 if ray_dirs is None else ray_dirs.shape[0]
    assert latents.is_contiguous() and directions.is_contiguous() and cond.shape[0] == U * D + R and xrow.shape[0] == U * D + R
    assert ray_dirs is None or (ray_dirs.is_contiguous() and ray_latent.dtype == torch.int64 and ray_latent.is_contiguous())
    check(_reni_in_fwd(ptr(latents), ptr(directions), U, L, D, ptr(ray_dirs), ptr(ray_latent), R, ptr(cond), ld(cond), ptr(xrow), ld(xrow),
                       stream_ptr()), "nsky_reni_grid_inputs_fwd")


def reni_grid_inputs_bwd(latents, directions, ray_dirs, ray_latent, d_cond, d_latents):
    U, L, _ = latents.shape
    D = directions.shape[0]
    R = 0 if ray_dirs is None else ray_dirs.shape[0]
    assert d_cond.shape[0] == U * D + R and d_latents.is_contiguous() and d_latents.shape == latents.shape
    check(_reni_in_bwd(ptr(latents), ptr(directions), U, L, D, ptr(ray_dirs), ptr(ray_latent), R, ptr(d_cond), ld(d_cond), ptr(d_latents),
                       stream_ptr()), "nsky_reni_grid_inputs_bwd")


_grid_probe = _sig("nsky_grid_probe_points", C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def grid_probe_points(lattice, gap, seed, counter, positions, directions):
    """lattice [P,3] (device), gap: three python floats; positions / directions [P,3] out; counter: int64 device tensor [1] (advanced)"""
    P = lattice.shape[0]
    assert lattice.is_contiguous() and positions.is_contiguous() and directions.is_contiguous() and positions.shape == (P, 3)
    assert counter.dtype == torch.int64 and counter.numel() == 1 and counter.is_cuda
    g3 = (C.c_float * 3)(*[float(v) for v in gap])
    check(_grid_probe(ptr(lattice), g3, P, int(seed) & (2**64 - 1), ptr(counter), ptr(positions), ptr(directions), stream_ptr()),
          "nsky_grid_probe_points")


_reni_out_fwd = _sig("nsky_reni_output_fwd", C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                     C.c_void_p)
_reni_out_bwd = _sig("nsky_reni_output_bwd", C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_void_p, C.c_void_p)


def reni_output_fwd(raw, scale, ray_latent, U, D, grid, rays):
    R = 0 if rays is None else rays.shape[0]
    assert raw.shape[0] == U * D + R and raw.stride(1) == 1 and scale.is_contiguous() and scale.numel() >= U
    assert grid.is_contiguous() and (rays is None or (rays.is_contiguous() and ray_latent.dtype == torch.int64 and ray_latent.is_contiguous()))
    check(_reni_out_fwd(ptr(raw), ld(raw), ptr(scale), ptr(ray_latent), U, D, R, ptr(grid), ptr(rays), stream_ptr()), "nsky_reni_output_fwd")


def reni_output_bwd(raw, scale, ray_latent, U, D, R, d_grid, d_rays, d_raw, d_scale):
    assert d_raw.shape == raw.shape and d_raw.is_contiguous() and raw.is_contiguous()
    assert (d_grid is None or d_grid.is_contiguous()) and (d_rays is None or d_rays.is_contiguous())
    check(_reni_out_bwd(ptr(raw), ld(raw), ptr(scale), ptr(ray_latent), U, D, R, ptr(d_grid), ptr(d_rays), ptr(d_raw), ptr(d_scale), stream_ptr()),
          "nsky_reni_output_bwd")


# ------------------------------------------------------------------------------------------ render stages
_P = C.c_void_p
_I = C.c_int32
_F = C.c_float
_hemi_fwd = _sig("nsky_hemi_composite_fwd", _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P)
_hemi_bwd = _sig("nsky_hemi_composite_bwd", _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P)
_neus_fwd = _sig("nsky_neus_weights_fwd", _P, _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P)
_neus_bwd = _sig("nsky_neus_weights_bwd", _P, _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P)
_neus_cos_fwd = _sig("nsky_neus_weights_cos_fwd", _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P)
_neus_cos_bwd = _sig("nsky_neus_weights_cos_bwd", _P, _P, _P, _P, _P, _F, _I, _I, _P, _P, _P, _P, _P, _P)
_vis_rays = _sig("nsky_visibility_rays", _P, _P, _P, _P, _I, _I, _F, _P, _P, _I, _P, _P, _P)
_vis_fin_fwd = _sig("nsky_visibility_finish_fwd", _P, _P, _P, _F, _P, _I, _I, _I, _P, _P)
_vis_fin_bwd = _sig("nsky_visibility_finish_bwd", _P, _P, _P, _F, _P, _I, _I, _I, _P, _P, _P, _P)


def _c(t):
    assert t is None or t.is_contiguous(), "contiguous tensor required"
    return ptr(t)


def hemi_composite_fwd(albedo, normals, weights, dirs, cam_colours, cam_of_ray, vis, bg, rgb, lin):
    R, S, _ = albedo.shape
    D = dirs.shape[0]
    assert cam_of_ray.dtype == torch.int32
    check(_hemi_fwd(_c(albedo), _c(normals), _c(weights), _c(dirs), _c(cam_colours), _c(cam_of_ray), _c(vis), _c(bg), R, S, D,
                    _c(rgb), _c(lin), stream_ptr()), "nsky_hemi_composite_fwd")


def hemi_composite_bwd(albedo, normals, weights, dirs, cam_colours, cam_of_ray, vis, bg, lin, d_rgb, d_albedo, d_normals,
                       d_weights, d_cam_colours, d_vis, d_bg):
    R, S, _ = albedo.shape
    D = dirs.shape[0]
    check(_hemi_bwd(_c(albedo), _c(normals), _c(weights), _c(dirs), _c(cam_colours), _c(cam_of_ray), _c(vis), _c(bg), _c(lin),
                    _c(d_rgb), R, S, D, _c(d_albedo), _c(d_normals), _c(d_weights), _c(d_cam_colours), _c(d_vis), _c(d_bg),
                    stream_ptr()), "nsky_hemi_composite_bwd")


def neus_weights_fwd(sdf, grad, ray_dirs, starts, ends, variance, anneal, alpha, weights, trans_bg, acc, depth):
    R, S = sdf.shape
    check(_neus_fwd(_c(sdf), _c(grad), _c(ray_dirs), _c(starts), _c(ends), _c(variance), anneal, R, S, _c(alpha), _c(weights),
                    _c(trans_bg), _c(acc), _c(depth), stream_ptr()), "nsky_neus_weights_fwd")


def neus_weights_bwd(sdf, grad, ray_dirs, starts, ends, variance, anneal, d_weights, d_trans_bg, d_sdf, d_grad, d_variance):
    R, S = sdf.shape
    check(_neus_bwd(_c(sdf), _c(grad), _c(ray_dirs), _c(starts), _c(ends), _c(variance), anneal, R, S, _c(d_weights),
                    _c(d_trans_bg), _c(d_sdf), _c(d_grad), _c(d_variance), stream_ptr()), "nsky_neus_weights_bwd")


def neus_weights_cos_fwd(sdf, cosv, starts, ends, variance, anneal, alpha, weights, trans_bg, acc, depth):
    """neus_weights_fwd with the gradient as one precomputed column cosv [R, S] = ray_dir . grad(sdf)"""
    R, S = sdf.shape
    assert cosv.numel() == R * S
    check(_neus_cos_fwd(_c(sdf), _c(cosv), _c(starts), _c(ends), _c(variance), anneal, R, S, _c(alpha), _c(weights), _c(trans_bg), _c(acc),
                        _c(depth), stream_ptr()), "nsky_neus_weights_cos_fwd")


def neus_weights_cos_bwd(sdf, cosv, starts, ends, variance, anneal, d_weights, d_trans_bg, d_sdf, d_cos, d_variance):
    R, S = sdf.shape
    assert cosv.numel() == R * S and d_cos.numel() == R * S
    check(_neus_cos_bwd(_c(sdf), _c(cosv), _c(starts), _c(ends), _c(variance), anneal, R, S, _c(d_weights), _c(d_trans_bg), _c(d_sdf),
                        _c(d_cos), _c(d_variance), stream_ptr()), "nsky_neus_weights_cos_bwd")


_ray_reduce_fwd = _sig("nsky_ray_reduce_fwd", _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P)
_ray_reduce_bwd = _sig("nsky_ray_reduce_bwd", _P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P, _P)
_normalize3_fwd = _sig("nsky_normalize3_fwd", _P, C.c_int64, _P, _P)
_normalize3_bwd = _sig("nsky_normalize3_bwd", _P, _P, C.c_int64, _P, _P)


def ray_reduce_fwd(weights, starts, ends, normals, albedo, max_clamp, sums, bounds, p2p, accumulation, normal, albedo_acc):
    R, S = weights.shape
    check(_ray_reduce_fwd(_c(weights), _c(starts), _c(ends), _c(normals), _c(albedo), R, S, float(max_clamp), _c(sums), _c(bounds), _c(p2p),
                          _c(accumulation), _c(normal), _c(albedo_acc), stream_ptr()), "nsky_ray_reduce_fwd")


def ray_reduce_bwd(weights, starts, ends, normals, albedo, sums, bounds, max_clamp, d_p2p, d_accumulation, d_normal, d_albedo_acc,
                   d_weights, d_normals, d_albedo):
    R, S = weights.shape
    check(_ray_reduce_bwd(_c(weights), _c(starts), _c(ends), _c(normals), _c(albedo), _c(sums), _c(bounds), R, S, float(max_clamp),
                          _c(d_p2p), _c(d_accumulation), _c(d_normal), _c(d_albedo_acc), _c(d_weights), _c(d_normals), _c(d_albedo),
                          stream_ptr()), "nsky_ray_reduce_bwd")


def normalize3_fwd(g, n):
    check(_normalize3_fwd(_c(g), g.numel() // 3, _c(n), stream_ptr()), "nsky_normalize3_fwd")


def normalize3_bwd(g, d_n, d_g):
    check(_normalize3_bwd(_c(g), _c(d_n), g.numel() // 3, _c(d_g), stream_ptr()), "nsky_normalize3_bwd")


def visibility_rays(origins, ray_dirs, depth, sel_dirs, radius, sphere_pts, xrow, surf_dist, term_dist=None):
    R, Dv = origins.shape[0], sel_dirs.shape[0]
    check(_vis_rays(_c(origins), _c(ray_dirs), _c(depth), _c(sel_dirs), R, Dv, radius, _c(sphere_pts), _c(xrow), ld(xrow),
                    _c(surf_dist), _c(term_dist), stream_ptr()), "nsky_visibility_rays")


def visibility_finish_fwd(t_hat, surf_dist, threshold, scale, sel_index, R, Dv, D, vis):
    assert sel_index.dtype == torch.int32
    check(_vis_fin_fwd(_c(t_hat), _c(surf_dist), _c(threshold), scale, _c(sel_index), R, Dv, D, _c(vis), stream_ptr()),
          "nsky_visibility_finish_fwd")


def visibility_finish_bwd(t_hat, surf_dist, threshold, scale, sel_index, R, Dv, D, d_vis, d_t_hat, d_threshold):
    check(_vis_fin_bwd(_c(t_hat), _c(surf_dist), _c(threshold), scale, _c(sel_index), R, Dv, D, _c(d_vis), _c(d_t_hat),
                       _c(d_threshold), stream_ptr()), "nsky_visibility_finish_bwd")


# ------------------------------------------------------------------------------------------ elementwise helpers
_sp_tan_bwd = _sig("nsky_softplus_tangent_bwd", _P, _P, _P, _P, _P, _P, _F, _I, _I, _I, _P, _P, _P, _P)
_pdf_sample = _sig("nsky_pdf_sample", _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P)
_adam = _sig("nsky_adam_step", _P, _P, _P, _P, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, _I, _F, _P)
_wn_fwd = _sig("nsky_weight_norm_fwd", _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P)
_wn_bwd = _sig("nsky_weight_norm_bwd", _P, _I, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P)


def softplus_tangent_bwd(da, s, ta, dta, ggrad, wvec, beta, N, Cc, dz, du, wsum=None):
    """wsum [Cc] (outer-product form): += sum_{n,k} ggrad[n,k] ta_k[n,:], the gradient of wvec, from the same pass"""
    check(_sp_tan_bwd(ptr(da), ptr(s), ptr(ta), ptr(dta), ptr(ggrad), ptr(wvec), beta, N, Cc, ld(s), ptr(dz), ptr(du), ptr(wsum),
                      stream_ptr()), "nsky_softplus_tangent_bwd")


def pdf_sample(weights, bins, u_base, jitter, num_bins, histogram_padding=0.01, eps=1e-5, want_inds=False):
    R, n0 = weights.shape
    assert bins.shape == (R, n0 + 1) and u_base.shape == (num_bins,)
    new_bins = torch.empty(R, num_bins, device=weights.device)
    inds = torch.empty(R, num_bins, dtype=torch.int32, device=weights.device) if want_inds else None
    check(_pdf_sample(_c(weights), _c(bins), _c(u_base), _c(jitter), R, n0, num_bins, histogram_padding, eps, _c(new_bins),
                      _c(inds), stream_ptr()), "nsky_pdf_sample")
    return new_bins, inds


_il_fwd = _sig("nsky_interlevel_fwd", _P, _P, _P, _P, _I, _I, _I, _P, _P)
_il_bwd = _sig("nsky_interlevel_bwd", _P, _P, _P, _P, _P, _I, _I, _I, _P, _P)


def interlevel_fwd(c, w, sb, wp, per_ray):
    R, S = w.shape
    check(_il_fwd(_c(c), _c(w), _c(sb), _c(wp), R, S, wp.shape[1], _c(per_ray), stream_ptr()), "nsky_interlevel_fwd")
    return per_ray


def interlevel_bwd(c, w, sb, wp, d_per_ray, d_wp):
    R, S = w.shape
    check(_il_bwd(_c(c), _c(w), _c(sb), _c(wp), _c(d_per_ray), R, S, wp.shape[1], _c(d_wp), stream_ptr()), "nsky_interlevel_bwd")
    return d_wp


_collider = _sig("nsky_sphere_collider", _P, _P, _I, _F, _F, _P, _P, _P)
_ubins = _sig("nsky_uniform_bins", _P, _P, _P, _I, _I, _P, _P, _P)
_b2s = _sig("nsky_bins_to_samples", _P, _P, _P, _P, _P, _I, _I, _P, _P, _P)


def sphere_collider(origins, directions, radius, near_plane):
    """origins, directions [R,3] -> nears, fars [R,1] (nerfstudio SphereCollider)"""
    R = origins.shape[0]
    nears = torch.empty(R, 1, device=origins.device)
    fars = torch.empty(R, 1, device=origins.device)
    check(_collider(_c(origins), _c(directions), R, radius, near_plane, ptr(nears), ptr(fars), stream_ptr()), "nsky_sphere_collider")
    return nears, fars


def uniform_bins(nears, fars, n, jitter):
    """-> sbins, ebins [R,n+1] (UniformSampler, single jitter per ray or None)"""
    R = nears.shape[0]
    sbins = torch.empty(R, n + 1, device=nears.device)
    ebins = torch.empty(R, n + 1, device=nears.device)
    check(_ubins(_c(nears), _c(fars), _c(jitter), R, n, ptr(sbins), ptr(ebins), stream_ptr()), "nsky_uniform_bins")
    return sbins, ebins


def bins_to_samples(sbins, nears, fars, origins=None, directions=None, want_ebins=True, want_positions=False):
    """sbins [R,n+1] -> (ebins [R,n+1] | None, positions [R,n,3] | None)"""
    R, n = sbins.shape[0], sbins.shape[1] - 1
    ebins = torch.empty(R, n + 1, device=sbins.device) if want_ebins else None
    pos = torch.empty(R, n, 3, device=sbins.device) if want_positions else None
    check(_b2s(_c(sbins), _c(nears), _c(fars), _c(origins), _c(directions), R, n, ptr(ebins), ptr(pos), stream_ptr()),
          "nsky_bins_to_samples")
    return ebins, pos


_dw_fwd = _sig("nsky_density_weights_fwd", _P, _I, _P, _I, _I, _P, _P)
_dw_bwd = _sig("nsky_density_weights_bwd", _P, _I, _P, _P, _I, _I, _P, _P)


def density_weights_fwd(raw, ebins, weights):
    """raw [R*n, ld] (column 0 = density-head output), ebins [R,n+1] -> weights [R,n]"""
    R, n = weights.shape
    check(_dw_fwd(ptr(raw), ld(raw), _c(ebins), R, n, _c(weights), stream_ptr()), "nsky_density_weights_fwd")
    return weights


def density_weights_bwd(raw, ebins, d_weights, d_raw):
    R, n = d_weights.shape
    check(_dw_bwd(ptr(raw), ld(raw), _c(ebins), _c(d_weights), R, n, _c(d_raw), stream_ptr()), "nsky_density_weights_bwd")
    return d_raw


def weight_norm_fwd(v, g, row_map, col_map, out, inv_norm):
    """out[r,c] = g[sr] v[sr,sc] / ||v[sr]|| under the row / column maps (int32, -1 = zero); see include/neusky_hip.h"""
    check(_wn_fwd(ptr(v), ptr(g), row_map.numel(), col_map.numel(), v.shape[1], ld(v), ptr(row_map), ptr(col_map), ptr(out),
                  ld(out), ptr(inv_norm), stream_ptr()), "nsky_weight_norm_fwd")
    return out


def weight_norm_bwd(d_out, v, g, inv_norm, row_map, inverse_col, dv, dg):
    check(_wn_bwd(ptr(d_out), ld(d_out), ptr(v), ptr(g), ptr(inv_norm), row_map.numel(), v.shape[1], ld(v), ptr(row_map),
                  ptr(inverse_col), ptr(dv), ptr(dg), stream_ptr()), "nsky_weight_norm_bwd")


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    n = p.numel()
    assert p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
    check(_adam(ptr(p), ptr(g), ptr(m), ptr(v), n, lr, beta1, beta2, eps, step, grad_scale, stream_ptr()), "nsky_adam_step")


# ------------------------------------------------------------------------------------------ attention core (RENI++ transformer decoder)
_attn_fwd = _sig("nsky_attn_core_fwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_attn_bwd = _sig("nsky_attn_core_bwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_add_ln_fwd = _sig("nsky_add_layer_norm_fwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_void_p)
_add_ln_bwd = _sig("nsky_add_layer_norm_bwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p)


def add_layer_norm_fwd(x, r, gamma, beta, eps, s, y, stats):
    """s = x + r (r None: s = x, not stored), y = LayerNorm(s), stats [M, 2] = (mean, rstd); x, r, s, y [M, W] contiguous"""
    M, W = x.shape
    assert all(t is None or t.is_contiguous() for t in (x, r, gamma, beta, s, y, stats))
    check(_add_ln_fwd(ptr(x), ptr(r), ptr(gamma), ptr(beta), M, W, float(eps), ptr(s), ptr(y), ptr(stats), stream_ptr()), "nsky_add_layer_norm_fwd")


def add_layer_norm_bwd(s, stats, gamma, dy, ds_in, ds):
    M, W = s.shape
    assert all(t is None or t.is_contiguous() for t in (s, stats, gamma, dy, ds_in, ds))
    check(_add_ln_bwd(ptr(s), ptr(stats), ptr(gamma), ptr(dy), ptr(ds_in), M, W, ptr(ds), stream_ptr()), "nsky_add_layer_norm_bwd")


_attn_rays_fwd = _sig("nsky_attn_core_rays_fwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                      C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_attn_rays_bwd = _sig("nsky_attn_core_rays_bwd", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def attn_core_rays_fwd(Q, dirs, perm, seg, Kt, Vt, scale, O, row_max, row_sum):
    """the rays' rows, sorted by camera (perm [R] int32, seg [U + 1] int32): Q / O [R, 16 nh], dirs [R, 3], row_max / row_sum [R, nh]"""
    R, H = Q.shape
    U, nh, L = Kt.shape[0], Kt.shape[1], Kt.shape[2]
    assert H == 16 * nh and perm.dtype == torch.int32 and seg.dtype == torch.int32 and seg.numel() == U + 1
    assert all(t.is_contiguous() for t in (Q, dirs, perm, seg, Kt, Vt, O, row_max, row_sum))
    check(_attn_rays_fwd(ptr(Q), ptr(dirs), ptr(perm), ptr(seg), ptr(Kt), ptr(Vt), U, R, L, nh, float(scale), ptr(O), ptr(row_max), ptr(row_sum),
                         stream_ptr()), "nsky_attn_core_rays_fwd")
    return O


def attn_core_rays_bwd(Q, dirs, perm, seg, Kt, Vt, O, row_max, row_sum, dO, scale, dQ, dKt, dVt):
    """adds the rays' part to dKt / dVt (call after attn_core_bwd on the same stream)"""
    R, H = Q.shape
    U, nh, L = Kt.shape[0], Kt.shape[1], Kt.shape[2]
    assert all(t.is_contiguous() for t in (Q, dirs, perm, seg, Kt, Vt, O, row_max, row_sum, dO, dQ, dKt, dVt))
    check(_attn_rays_bwd(ptr(Q), ptr(dirs), ptr(perm), ptr(seg), ptr(Kt), ptr(Vt), ptr(O), ptr(row_max), ptr(row_sum), ptr(dO), U, R, L, nh,
                         float(scale), ptr(dQ), ptr(dKt), ptr(dVt), stream_ptr()), "nsky_attn_core_rays_bwd")


def attn_core_fwd(Q, dirs, Kt, Vt, scale, O, row_max, row_sum):
    """Q [U,D,16 nh], dirs [U,D,3], Kt / Vt [U,nh,L,48] -> O [U,D,16 nh], row_max / row_sum [U,nh,D] (include/neusky_hip.h)"""
    U, D, H = Q.shape
    nh, L = Kt.shape[1], Kt.shape[2]
    assert H == 16 * nh and Kt.shape[3] == 48 and all(t.is_contiguous() for t in (Q, dirs, Kt, Vt, O, row_max, row_sum))
    check(_attn_fwd(ptr(Q), ptr(dirs), ptr(Kt), ptr(Vt), U, D, L, nh, float(scale), ptr(O), ptr(row_max), ptr(row_sum), stream_ptr()),
          "nsky_attn_core_fwd")
    return O


def attn_core_bwd(Q, dirs, Kt, Vt, O, row_max, row_sum, dO, scale, dQ, dKt, dVt):
    U, D, H = Q.shape
    nh, L = Kt.shape[1], Kt.shape[2]
    assert all(t.is_contiguous() for t in (Q, dirs, Kt, Vt, O, row_max, row_sum, dO, dQ, dKt, dVt))
    # D = dO . O per row and head (from the row kernel to the token kernel), then four floats per (camera, head): the operand maxima
    drow = torch.empty(U * nh * (D + 4), device=Q.device)
    check(_attn_bwd(ptr(Q), ptr(dirs), ptr(Kt), ptr(Vt), ptr(O), ptr(row_max), ptr(row_sum), ptr(dO), U, D, L, nh, float(scale),
                    ptr(dQ), ptr(dKt), ptr(dVt), ptr(drow), stream_ptr()), "nsky_attn_core_bwd")


# ------------------------------------------------------------------------------------------ fused loss terms
TOTAL_MAX_SEGMENTS = 8


class TotalSegment(C.Structure):
    _fields_ = [("x", C.c_void_p), ("coef", C.c_void_p), ("grad", C.c_void_p), ("n", C.c_int32), ("scale", C.c_float)]


_total_fwd = _sig("nsky_weighted_total_fwd", C.POINTER(TotalSegment), C.c_int32, C.c_void_p, C.c_void_p)
_total_bwd = _sig("nsky_weighted_total_bwd", C.POINTER(TotalSegment), C.c_int32, C.c_void_p, C.c_void_p)


def weighted_total_fwd(parts, total):
    """parts: [(x, coef | None, scale)] -> total[0] = sum_s scale_s sum_i coef_s[i] x_s[i] (one launch; include/neusky_hip.h)"""
    assert 0 < len(parts) <= TOTAL_MAX_SEGMENTS
    arr = (TotalSegment * len(parts))(*[TotalSegment(ptr(x), ptr(c), None, x.numel(), float(sc)) for x, c, sc in parts])
    check(_total_fwd(arr, len(parts), ptr(total), stream_ptr()), "nsky_weighted_total_fwd")
    return total


def weighted_total_bwd(parts, g, grads):
    """grads[s] (or None) = g[0] scale_s coef_s"""
    arr = (TotalSegment * len(parts))(*[TotalSegment(ptr(x), ptr(c), ptr(d), x.numel(), float(sc)) for (x, c, sc), d in zip(parts, grads)])
    check(_total_bwd(arr, len(parts), ptr(g), stream_ptr()), "nsky_weighted_total_bwd")


class MainLossesDesc(C.Structure):
    _fields_ = [("R", C.c_int32), ("S", C.c_int32), ("P", C.c_int32), ("M", C.c_int32),
                ("rgb", C.c_void_p), ("image", C.c_void_p), ("mask", C.c_void_p), ("eik", C.c_void_p), ("weights", C.c_void_p),
                ("normal", C.c_void_p), ("hdr_bg", C.c_void_p), ("grid", C.c_void_p), ("sdf_term", C.c_void_p), ("vis_thr", C.c_void_p),
                ("sky_alpha", C.c_float), ("vis_target", C.c_float)]


class DDFLossesDesc(C.Structure):
    _fields_ = [("Mr", C.c_int32), ("Mm", C.c_int32), ("Ms", C.c_int32),
                ("expected", C.c_void_p), ("term", C.c_void_p), ("mask", C.c_void_p), ("dist_weight", C.c_void_p), ("sdf", C.c_void_p),
                ("mv_expected", C.c_void_p), ("mv_term", C.c_void_p), ("sky_expected", C.c_void_p), ("sky_term", C.c_void_p),
                ("want_depth", C.c_int32), ("want_sdf_l2", C.c_int32), ("want_sdf_l1", C.c_int32), ("mask_to_circumference", C.c_int32),
                ("inverse_depth_weight", C.c_int32), ("radius", C.c_float)]


_main_losses_fwd = _sig("nsky_main_losses_fwd", C.POINTER(MainLossesDesc), C.c_void_p, C.c_void_p, C.c_void_p)
_main_losses_bwd = _sig("nsky_main_losses_bwd", C.POINTER(MainLossesDesc), *([C.c_void_p] * 11))
_ddf_losses_fwd = _sig("nsky_ddf_losses_fwd", C.POINTER(DDFLossesDesc), C.c_void_p, C.c_void_p)
_ddf_losses_bwd = _sig("nsky_ddf_losses_bwd", C.POINTER(DDFLossesDesc), *([C.c_void_p] * 8))
N_MAIN_TERMS, N_DDF_TERMS = 8, 5


def main_losses_fwd(desc: MainLossesDesc, terms, wsum):
    check(_main_losses_fwd(C.byref(desc), ptr(terms), ptr(wsum), stream_ptr()), "nsky_main_losses_fwd")


def main_losses_bwd(desc: MainLossesDesc, wsum, d_terms, d_rgb, d_eik, d_weights, d_normal, d_hdr_bg, d_grid, d_sdf_term, d_vis_thr):
    check(_main_losses_bwd(C.byref(desc), ptr(wsum), ptr(d_terms), ptr(d_rgb), ptr(d_eik), ptr(d_weights), ptr(d_normal), ptr(d_hdr_bg),
                           ptr(d_grid), ptr(d_sdf_term), ptr(d_vis_thr), stream_ptr()), "nsky_main_losses_bwd")


def ddf_losses_fwd(desc: DDFLossesDesc, terms):
    check(_ddf_losses_fwd(C.byref(desc), ptr(terms), stream_ptr()), "nsky_ddf_losses_fwd")


def ddf_losses_bwd(desc: DDFLossesDesc, d_terms, d_expected, d_sdf, d_mv_expected, d_sky_expected, d_term, d_mv_term):
    check(_ddf_losses_bwd(C.byref(desc), ptr(d_terms), ptr(d_expected), ptr(d_sdf), ptr(d_mv_expected), ptr(d_sky_expected), ptr(d_term),
                          ptr(d_mv_term), stream_ptr()), "nsky_ddf_losses_bwd")


# ------------------------------------------------------------------------------------------ fused FiLM-SIREN chain
FILM_MAX_LAYERS = 12
FILM_TABLE_FLOATS = 6656  # biases + reciprocal tile scales written by nsky_film_pack
FILM_SAVED_WIDTHS = (256,)  # hidden widths whose chain runs on saved FiLM operands by default (film_saved_operands)


class FilmNet(C.Structure):
    _fields_ = [("hidden", C.c_int32), ("n_map", C.c_int32), ("n_film", C.c_int32),
                ("cond_dim", C.c_int32), ("x_dim", C.c_int32), ("out_dim", C.c_int32),
                ("map_w", C.c_void_p * FILM_MAX_LAYERS), ("map_b", C.c_void_p * FILM_MAX_LAYERS), ("map_ld", C.c_int32 * FILM_MAX_LAYERS),
                ("mo_w", C.c_void_p), ("mo_b", C.c_void_p), ("mo_ld", C.c_int32),
                ("film_w", C.c_void_p * FILM_MAX_LAYERS), ("film_b", C.c_void_p * FILM_MAX_LAYERS), ("film_ld", C.c_int32 * FILM_MAX_LAYERS),
                ("out_w", C.c_void_p), ("out_b", C.c_void_p), ("out_ld", C.c_int32)]


_film_layout = _sig("nsky_film_stream_layout", C.POINTER(FilmNet), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32))
_film_pack = _sig("nsky_film_pack", C.POINTER(FilmNet), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_film_fwd = _sig("nsky_film_chain_fwd", C.POINTER(FilmNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)


_film_bwd_film = _sig("nsky_film_chain_bwd_film", C.POINTER(FilmNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)
_film_fwd_saved = _sig("nsky_film_chain_fwd_saved", C.POINTER(FilmNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                       C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p)
_film_bwd_film_saved = _sig("nsky_film_chain_bwd_film_saved", C.POINTER(FilmNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                            C.c_void_p)
_film_bwd_map = _sig("nsky_film_chain_bwd_map", C.POINTER(FilmNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)


_wgrad_native = _sig("nsky_wgrad_native", C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                     C.c_void_p, C.c_float, C.c_void_p)


class WgradProblem(C.Structure):
    _fields_ = [("dZ", C.c_void_p), ("nnt_a", C.c_int32), ("X", C.c_void_p), ("nnt_b", C.c_int32), ("dW", C.c_void_p), ("ldw", C.c_int32),
                ("db", C.c_void_p), ("a_scale_max", C.c_void_p), ("b_scale", C.c_float),
                ("lda", C.c_int32), ("ldb", C.c_int32), ("width_a", C.c_int32), ("width_b", C.c_int32), ("bias_rows", C.c_int32),
                ("bias_row_mod", C.c_int32), ("b_scale_max", C.c_void_p)]


WGRAD_MAX_PROBLEMS = 16
_wgrad_native_batch = _sig("nsky_wgrad_native_batch", C.POINTER(WgradProblem), C.c_int32, C.c_int32, C.c_void_p)


def wgrad_problem(dZ, nnt_a, X, nnt_b, rows, dW, db=None, a_scale_max=None, b_scale=64.0, width_a=0, width_b=0, bias_row_mod=0,
                  b_scale_max=None) -> WgradProblem:
    """width_a / width_b: features of dZ / X that exist when fewer than the tiles walked (dW is then [width_a, width_b]);
    bias_row_mod = 4: db sums the value rows (row % 4 == 0) of a quad-native dZ only; b_scale_max: device scalar max |X| (replaces the
    constant b_scale: operands that carry input tangents have no a-priori bound)"""
    wa, wb = width_a or 32 * nnt_a, width_b or 32 * nnt_b
    assert dW.stride(1) == 1 and dW.shape[0] >= wa and dW.shape[1] >= wb
    assert dZ.numel() >= film_rows(rows) * 32 * nnt_a and X.numel() >= film_rows(rows) * 32 * nnt_b
    return WgradProblem(ptr(dZ), nnt_a, ptr(X), nnt_b, ptr(dW), ld(dW), ptr(db), ptr(a_scale_max), float(b_scale), 0, 0, int(width_a), int(width_b), 0,
                        int(bias_row_mod), ptr(b_scale_max))


def wgrad_problem_rowmajor(dZ, n_out, X, k_in, rows, dW, db=None, bias_rows=0) -> WgradProblem:
    """dW[n_out, k_in] += dZ[:rows, :n_out]^T X[:rows, :k_in] over ROW-MAJOR operands (2-term bf16 products); see include/neusky_hip.h"""
    assert dW.stride(1) == 1 and dW.shape[0] >= n_out and dW.shape[1] >= k_in and n_out % 4 == 0 and k_in % 4 == 0
    assert dZ.shape[0] >= rows and X.shape[0] >= rows and ld(dZ) >= n_out and ld(X) >= k_in
    return WgradProblem(ptr(dZ), 0, ptr(X), 0, ptr(dW), ld(dW), ptr(db), None, 1.0, ld(dZ), ld(X), n_out, k_in, int(bias_rows), 0, None)


def wgrad_native_batch(problems, rows):
    """every problem: dW += dZ^T X, db += column sums of dZ over tile-native matrices sharing the batch `rows`; ONE launch
    (csrc/wgrad_native.hip).  problems: list of wgrad_problem(...), at most WGRAD_MAX_PROBLEMS."""
    for i in range(0, len(problems), WGRAD_MAX_PROBLEMS):
        chunk = problems[i:i + WGRAD_MAX_PROBLEMS]
        arr = (WgradProblem * len(chunk))(*chunk)
        check(_wgrad_native_batch(arr, len(chunk), rows, stream_ptr()), "nsky_wgrad_native_batch")


def wgrad_native(dZ, nnt_a, X, nnt_b, rows, dW, db=None, a_scale_max=None, b_scale=64.0):
    """dW[32 nnt_a, 32 nnt_b] += dZ^T X and db += column sums of dZ over two tile-native matrices (csrc/wgrad_native.hip);
    dW / db are accumulated into.  nnt_a, nnt_b: multiples of 4."""
    wgrad_problem(dZ, nnt_a, X, nnt_b, rows, dW, db, a_scale_max, b_scale)  # shape checks
    check(_wgrad_native(ptr(dZ), nnt_a, ptr(X), nnt_b, rows, ptr(dW), ld(dW), ptr(db), ptr(a_scale_max), float(b_scale), stream_ptr()),
          "nsky_wgrad_native")
    return dW


def film_supported(hidden, map_hidden, n_map, n_film, cond_dim, x_dim, out_dim) -> bool:
    """shapes the fused chain kernels are built for (anything else runs the per-layer dense kernels)"""
    return (hidden in (128, 256) and map_hidden == hidden and 1 <= n_map <= FILM_MAX_LAYERS and 1 <= n_film <= FILM_MAX_LAYERS
            and 1 <= cond_dim <= 320 and 1 <= x_dim <= 16 and 1 <= out_dim <= 4
            and n_map * hidden + 3 * n_film * hidden + 32 <= 6144)


def film_net(cond_dim, x_dim, out_dim, map_w, map_b, mo_w, mo_b, film_w, film_b, out_w, out_b) -> FilmNet:
    """describe a FiLM-SIREN by its fp32 parameter tensors (torch nn.Linear layout, rows contiguous); the caller keeps
    the tensors alive while the descriptor is in use"""
    n = FilmNet(hidden=film_w[0].shape[0], n_map=len(map_w), n_film=len(film_w), cond_dim=cond_dim, x_dim=x_dim, out_dim=out_dim)
    for i, (w, b) in enumerate(zip(map_w, map_b)):
        n.map_w[i], n.map_b[i], n.map_ld[i] = ptr(w), ptr(b), ld(w)
    for i, (w, b) in enumerate(zip(film_w, film_b)):
        n.film_w[i], n.film_b[i], n.film_ld[i] = ptr(w), ptr(b), ld(w)
    n.mo_w, n.mo_b, n.mo_ld = ptr(mo_w), ptr(mo_b), ld(mo_w)
    n.out_w, n.out_b, n.out_ld = ptr(out_w), ptr(out_b), ld(out_w)
    return n


def film_stream_layout(net: FilmNet, direction: int = 0):
    nbytes, ntiles = C.c_int64(0), C.c_int32(0)
    check(_film_layout(C.byref(net), direction, C.byref(nbytes), C.byref(ntiles)), "nsky_film_stream_layout")
    return nbytes.value, ntiles.value


def film_pack(net: FilmNet, stream_buf, scales, direction: int = 0):
    check(_film_pack(C.byref(net), direction, ptr(stream_buf), ptr(scales), stream_ptr()), "nsky_film_pack")


_ray_points_fwd = _sig("nsky_ray_points_fwd", C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
_ray_points_bwd = _sig("nsky_ray_points_bwd", C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)


def ray_points_fwd(origins, dirs, sign, t, out):
    """out[i] = origins[i] + sign t[i] dirs[i % len(dirs)]; out may be a row slice of a larger [*, 3] buffer"""
    n = origins.shape[0]
    assert origins.is_contiguous() and dirs.is_contiguous() and t.is_contiguous() and out.is_contiguous() and out.shape == (n, 3) and t.numel() == n
    check(_ray_points_fwd(ptr(origins), ptr(dirs), dirs.shape[0], float(sign), ptr(t), n, ptr(out), stream_ptr()), "nsky_ray_points_fwd")


def ray_points_bwd(dirs, sign, d_out, d_t):
    n = d_out.shape[0]
    assert dirs.is_contiguous() and d_out.is_contiguous() and d_t.is_contiguous() and d_t.numel() == n
    check(_ray_points_bwd(ptr(dirs), dirs.shape[0], float(sign), ptr(d_out), n, ptr(d_t), stream_ptr()), "nsky_ray_points_bwd")


_train_metrics = _sig("nsky_train_metrics", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p)


def train_metrics(pred, gt, mask, peak_sq, variance=None):
    """-> out [3] float32: [PSNR-like 10 log10(peak_sq / mse of the (masked) difference), s_val, 1 / s_val] (the last two when
    variance is given); pred / gt / mask contiguous with the same number of elements"""
    n = pred.numel()
    assert pred.is_contiguous() and gt.is_contiguous() and gt.numel() == n and (mask is None or (mask.is_contiguous() and mask.numel() == n))
    assert pred.dtype == gt.dtype == torch.float32 and (mask is None or mask.dtype == torch.float32)
    out = torch.empty(3, device=pred.device)
    check(_train_metrics(ptr(pred), ptr(gt), ptr(mask), n, float(peak_sq), ptr(variance), ptr(out), stream_ptr()), "nsky_train_metrics")
    return out


_point_alphas_fwd = _sig("nsky_point_alphas_fwd", C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_float, C.c_int32,
                         C.c_void_p, C.c_void_p)
_point_alphas_bwd = _sig("nsky_point_alphas_bwd", C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p, C.c_float, C.c_int32,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def point_alphas_fwd(sdf, grad, dirs, gaps, variance, anneal, alphas):
    P = sdf.numel()
    assert sdf.is_contiguous() and grad.is_contiguous() and dirs.is_contiguous() and alphas.is_contiguous() and alphas.shape == (P, 3)
    g3 = (C.c_float * 3)(*[float(v) for v in gaps])
    check(_point_alphas_fwd(ptr(sdf), ptr(grad), ptr(dirs), g3, ptr(variance), float(anneal), P, ptr(alphas), stream_ptr()), "nsky_point_alphas_fwd")


def point_alphas_bwd(sdf, grad, dirs, gaps, variance, anneal, d_alphas, d_sdf, d_grad, d_variance):
    P = sdf.numel()
    assert d_alphas.is_contiguous() and d_sdf.is_contiguous() and d_grad.is_contiguous()
    g3 = (C.c_float * 3)(*[float(v) for v in gaps])
    check(_point_alphas_bwd(ptr(sdf), ptr(grad), ptr(dirs), g3, ptr(variance), float(anneal), P, ptr(d_alphas), ptr(d_sdf), ptr(d_grad),
                            ptr(d_variance), stream_ptr()), "nsky_point_alphas_bwd")


_sig_col_fwd = _sig("nsky_sigmoid_column_fwd", C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_void_p)
_sig_col_bwd = _sig("nsky_sigmoid_column_bwd", C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p)


def sigmoid_column_fwd(raw, scale, t):
    assert raw.dim() == 2 and raw.stride(1) == 1 and t.is_contiguous() and t.numel() == raw.shape[0]
    check(_sig_col_fwd(ptr(raw), ld(raw), raw.shape[0], float(scale), ptr(t), stream_ptr()), "nsky_sigmoid_column_fwd")


def sigmoid_column_bwd(raw, scale, d_t, d_raw):
    assert d_raw.shape == raw.shape and d_raw.is_contiguous() and raw.is_contiguous() and d_t.is_contiguous()
    check(_sig_col_bwd(ptr(raw), ld(raw), raw.shape[0], float(scale), ptr(d_t), ptr(d_raw), stream_ptr()), "nsky_sigmoid_column_bwd")


_prop_fwd = _sig("nsky_proposal_mlp_fwd", C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_void_p)
_prop_bwd = _sig("nsky_proposal_mlp_bwd", C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def proposal_mlp_supported(in_dim: int, hidden: int) -> bool:
    return hidden == 16 and 1 <= in_dim <= 12


def proposal_mlp_fwd(feat, w0, b0, w1, b1, raw):
    """feat [P, ld >= in_dim] -> raw [P]; w0 [16, in_dim], b0 [16], w1 [1, 16] or [16], b1 [1] (torch nn.Linear tensors)"""
    P, in_dim = feat.shape[0], w0.shape[1]
    assert feat.stride(1) == 1 and w0.is_contiguous() and w1.is_contiguous() and raw.is_contiguous() and raw.numel() == P
    check(_prop_fwd(ptr(feat), ld(feat), P, in_dim, w0.shape[0], ptr(w0), ld(w0), ptr(b0), ptr(w1), ptr(b1), ptr(raw), stream_ptr()),
          "nsky_proposal_mlp_fwd")


def proposal_mlp_bwd(feat, w0, b0, w1, b1, d_raw, d_feat, dw0, db0, dw1, db1):
    P, in_dim = feat.shape[0], w0.shape[1]
    assert d_raw.is_contiguous() and d_raw.numel() == P and (d_feat is None or (d_feat.shape == feat.shape and d_feat.is_contiguous() and feat.is_contiguous()))
    assert dw0.shape == w0.shape and dw0.is_contiguous()
    check(_prop_bwd(ptr(feat), ld(feat), P, in_dim, w0.shape[0], ptr(w0), ld(w0), ptr(b0), ptr(w1), ptr(b1), ptr(d_raw), ptr(d_feat), ptr(dw0),
                    ptr(db0), ptr(dw1), ptr(db1), stream_ptr()), "nsky_proposal_mlp_bwd")


class Segment(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int64)]


_gather_segments = _sig("nsky_gather_segments", C.POINTER(Segment), C.c_int32, C.c_void_p)


def gather_segments(pairs):
    """pairs: [(src, dst)] contiguous float32 tensors of equal numel: dst <- src for all of them in ONE launch"""
    if not pairs:
        return
    arr = (Segment * len(pairs))()
    for i, (src, dst) in enumerate(pairs):
        assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel() and src.dtype == dst.dtype == torch.float32
        arr[i] = Segment(src.data_ptr(), dst.data_ptr(), src.numel())
    check(_gather_segments(arr, len(pairs), stream_ptr()), "nsky_gather_segments")


_copy_segments = _sig("nsky_copy_segments", C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_void_p)


def copy_segments(pairs):
    """pairs: [(src, dst)] contiguous device tensors of equal dtype and numel: dst <- src for all of them in ONE launch"""
    if not pairs:
        return
    n = len(pairs)
    src, dst, nb = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)()
    for i, (s_, d_) in enumerate(pairs):
        assert s_.is_cuda and d_.is_cuda and s_.is_contiguous() and d_.is_contiguous() and s_.dtype == d_.dtype and s_.numel() == d_.numel()
        src[i], dst[i], nb[i] = s_.data_ptr(), d_.data_ptr(), s_.numel() * s_.element_size()
    check(_copy_segments(src, dst, nb, n, stream_ptr()), "nsky_copy_segments")


class SdfNet(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("hidden", C.c_int32),
                ("w0", C.c_void_p), ("ld0", C.c_int32), ("b0", C.c_void_p),
                ("w1", C.c_void_p), ("ld1", C.c_int32), ("b1", C.c_void_p),
                ("w2", C.c_void_p), ("b2", C.c_void_p), ("beta", C.c_float)]


_sdf_layout = _sig("nsky_sdf_stream_layout", C.POINTER(SdfNet), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32))
_sdf_pack = _sig("nsky_sdf_pack", C.POINTER(SdfNet), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_sdf_fwd = _sig("nsky_sdf_chain_fwd", C.POINTER(SdfNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_void_p)
_sdf_bwd = _sig("nsky_sdf_chain_bwd", C.POINTER(SdfNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def sdf_supported(in_dim: int, hidden: int) -> bool:
    return hidden == 256 and 4 <= in_dim <= 80 and in_dim % 4 == 0


def sdf_net(W0, b0, W1, b1, w2_row, b2_elem, beta) -> SdfNet:
    """the geometry network evaluated for its sdf only: W0 [hidden, in_dim], W1 [hidden, hidden], w2_row [hidden] (a contiguous
    row view), b2_elem a 1-element view; the caller keeps the tensors alive while the descriptor is in use"""
    return SdfNet(in_dim=W0.shape[1], hidden=W0.shape[0], w0=ptr(W0), ld0=ld(W0), b0=ptr(b0), w1=ptr(W1), ld1=ld(W1), b1=ptr(b1),
                  w2=ptr(w2_row), b2=ptr(b2_elem), beta=float(beta))


def sdf_stream_layout(net: SdfNet, direction: int = 0):
    nbytes, ntiles = C.c_int64(0), C.c_int32(0)
    check(_sdf_layout(C.byref(net), direction, C.byref(nbytes), C.byref(ntiles)), "nsky_sdf_stream_layout")
    return nbytes.value, ntiles.value


def sdf_pack(net: SdfNet, stream_buf, table, direction: int = 0):
    check(_sdf_pack(C.byref(net), direction, ptr(stream_buf), ptr(table), stream_ptr()), "nsky_sdf_pack")


def sdf_chain_fwd(net: SdfNet, stream_buf, table, E, M, a0_save, a1_save, sdf):
    check(_sdf_fwd(C.byref(net), ptr(stream_buf), ptr(table), ptr(E), ld(E), M, ptr(a0_save), ptr(a1_save), ptr(sdf), stream_ptr()),
          "nsky_sdf_chain_fwd")
    return sdf


def sdf_chain_bwd(net: SdfNet, stream_buf, table, M, g_sdf, a0_save, a1_save, dz1, dz0, dE, dw2, db2, gmax):
    check(_sdf_bwd(C.byref(net), ptr(stream_buf), ptr(table), M, ptr(g_sdf), ptr(a0_save), ptr(a1_save), ptr(dz1), ptr(dz0),
                   ptr(dE), 0 if dE is None else ld(dE), ptr(dw2), ptr(db2), ptr(gmax), stream_ptr()), "nsky_sdf_chain_bwd")


# ------------------------------------------------------------------------------------------ SDF / albedo field chain
CHAIN_MAX_LAYERS = 8


class ChainLayer(C.Structure):
    _fields_ = [("W", C.c_void_p), ("ld", C.c_int32), ("rows", C.c_int32), ("K", C.c_int32), ("transposed", C.c_int32)]


class FieldNet(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("npe", C.c_int32), ("beta", C.c_float),
                ("b0", C.c_void_p), ("b1", C.c_void_p), ("w_sdf", C.c_void_p), ("b_sdf", C.c_void_p), ("b2f", C.c_void_p),
                ("bc0", C.c_void_p), ("bc1", C.c_void_p), ("wc2", C.c_void_p), ("ldc2", C.c_int32), ("bc2", C.c_void_p)]


_chain_layout = _sig("nsky_chain_stream_layout", C.POINTER(ChainLayer), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32))
_chain_pack = _sig("nsky_chain_pack", C.POINTER(ChainLayer), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_field_geo_fwd = _sig("nsky_field_geo_fwd", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_field_col_fwd = _sig("nsky_field_colour_fwd", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_field_col_bwd = _sig("nsky_field_colour_bwd", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_field_geo_bwd = _sig("nsky_field_geo_bwd", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_native_wcolsum = _sig("nsky_native_weighted_colsum", C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                       C.c_int32, C.c_void_p, C.c_void_p)
_field_geo_fwd_dir = _sig("nsky_field_geo_fwd_dir", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_field_geo_bwd_dir = _sig("nsky_field_geo_bwd_dir", C.POINTER(FieldNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_native_wcolsum_pair = _sig("nsky_native_weighted_colsum_pair", C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p)


def chain_layer(W, rows, K, transposed=False) -> ChainLayer:
    """one layer of a packed weight stream: W[r][k] = W[r * ld + k] (transposed: W[k * ld + r]), r < rows, k < K"""
    return ChainLayer(ptr(W), ld(W), int(rows), int(K), int(bool(transposed)))


def chain_pack(layers, device, buffers=None):
    """-> (stream bytes tensor, per-tile reciprocal scales, number of groups); see include/neusky_hip.h.
    buffers(nbytes, n_scales) -> (zero-initialised uint8 stream buffer, scales buffer): a caller's persistent pair (the pack writes
    the real slabs only, so the pad slabs of a buffer that has held the same layout before are still zero)"""
    arr = (ChainLayer * len(layers))(*layers)
    nbytes, ntiles, ngroups = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    check(_chain_layout(arr, len(layers), C.byref(nbytes), C.byref(ntiles), C.byref(ngroups)), "nsky_chain_stream_layout")
    if buffers is not None:
        stream, scales = buffers(nbytes.value, max(ntiles.value, 4))
    else:
        stream = torch.zeros(nbytes.value, dtype=torch.uint8, device=device)  # (pad slabs of partial groups are streamed, never multiplied)
        scales = torch.empty(max(ntiles.value, 4), device=device)
    check(_chain_pack(arr, len(layers), ptr(stream), ptr(scales), stream_ptr()), "nsky_chain_pack")
    return stream, scales, ngroups.value


def field_supported(in_dim: int, hidden: int, geo_feat: int, hidden_colour: int, colour_in: int) -> bool:
    """shapes the fused field kernels are built for (the `neusky` method's, neusky_config.py:66-77)"""
    return hidden == 256 and geo_feat == 256 and hidden_colour == 256 and 68 <= in_dim <= 80 and in_dim % 4 == 0 and colour_in == 300


def field_net(in_dim, npe, beta, b0, b1, w_sdf, b_sdf, b2f=None, bc0=None, bc1=None, wc2=None, bc2=None) -> FieldNet:
    return FieldNet(in_dim=in_dim, npe=npe, beta=float(beta), b0=ptr(b0), b1=ptr(b1), w_sdf=ptr(w_sdf), b_sdf=ptr(b_sdf), b2f=ptr(b2f),
                    bc0=ptr(bc0), bc1=ptr(bc1), wc2=ptr(wc2), ldc2=0 if wc2 is None else ld(wc2), bc2=ptr(bc2))


def field_geo_fwd(net: FieldNet, pack, ET, N, a0q, a1q, Eq, a1max, sdf, grad, qmax=None):
    """qmax [2] (zero-filled by the caller): max |Eq|, max |a0q| -- the b_scale_max of the first two layers' weight gradients"""
    stream, scales, groups = pack
    check(_field_geo_fwd(C.byref(net), ptr(stream), ptr(scales), groups, ptr(ET), ld(ET), N, ptr(a0q), ptr(a1q), ptr(Eq), ptr(a1max), ptr(sdf),
                         ptr(grad), ptr(qmax), stream_ptr()), "nsky_field_geo_fwd")


def field_colour_fwd(net: FieldNet, pack, ET, N, a1q, a1max, a1v, feat, xpe, c0, c1, alb):
    stream, scales, groups = pack
    check(_field_col_fwd(C.byref(net), ptr(stream), ptr(scales), groups, ptr(ET), ld(ET), N, ptr(a1q), ptr(a1max), ptr(a1v), ptr(feat), ptr(xpe),
                         ptr(c0), ptr(c1), ptr(alb), stream_ptr()), "nsky_field_colour_fwd")


def field_colour_bwd(net: FieldNet, pack, N, g_alb, alb, c0, c1, dpc2, dpc1, dpc0, dfeat, dxpe, da1v, gmax):
    stream, scales, groups = pack
    check(_field_col_bwd(C.byref(net), ptr(stream), ptr(scales), groups, N, ptr(g_alb), ptr(alb), ptr(c0), ptr(c1), ptr(dpc2), ptr(dpc1), ptr(dpc0),
                         ptr(dfeat), ptr(dxpe), ptr(da1v), ptr(gmax), stream_ptr()), "nsky_field_colour_bwd")


def field_geo_bwd(net: FieldNet, pack, N, g_sdf, g_grad, da1v, dxpe, a0q, a1q, d1q, d0q, dET, gmax):
    stream, scales, groups = pack
    check(_field_geo_bwd(C.byref(net), ptr(stream), ptr(scales), groups, N, ptr(g_sdf), ptr(g_grad), ptr(da1v), ptr(dxpe), ptr(a0q), ptr(a1q),
                         ptr(d1q), ptr(d0q), ptr(dET), 0 if dET is None else ld(dET), ptr(gmax), stream_ptr()), "nsky_field_geo_bwd")


def native_weighted_colsum(X, nt, rows, out, bias=None, w4=None, n_out=1, g_sdf=None, g_grad=None):
    """out[o] += sum_rows w[row][o] X[row] over a tile-native X [rows, 32 nt]; w4 [rows, 4], or the quad form (g_sdf / g_grad)"""
    check(_native_wcolsum(ptr(X), nt, rows, ptr(w4), n_out, ptr(g_sdf), ptr(g_grad), ptr(out), ld(out) if out.dim() == 2 else out.shape[0],
                          ptr(bias), stream_ptr()), "nsky_native_weighted_colsum")


def field_geo_fwd_dir(net: FieldNet, pack, ET, N, a0q, a1q, Eq, sdf, cosv, qmax=None):
    """the directional (pair-layout) geometry forward: ET stacked [E; Td] [2 N, ld]; sdf [N], cosv [N]; a0q / a1q / Eq pair-native"""
    stream, scales, groups = pack
    assert ET.shape[0] == 2 * N and sdf.numel() == N and cosv.numel() == N and a0q.shape[0] >= film_rows(2 * N) and a1q.shape[0] >= film_rows(2 * N)
    assert Eq is None or Eq.shape[0] >= film_rows(2 * N)
    check(_field_geo_fwd_dir(C.byref(net), ptr(stream), ptr(scales), groups, ptr(ET), ld(ET), N, ptr(a0q), ptr(a1q), ptr(Eq), ptr(sdf), ptr(cosv),
                             ptr(qmax), stream_ptr()), "nsky_field_geo_fwd_dir")


def field_geo_bwd_dir(net: FieldNet, pack, N, g_sdf, g_cos, a0q, a1q, d1q, d0q, dET, gmax):
    stream, scales, groups = pack
    assert (g_sdf is None or g_sdf.numel() == N) and (g_cos is None or g_cos.numel() == N) and (dET is None or dET.shape[0] == 2 * N)
    assert min(a0q.shape[0], a1q.shape[0], d1q.shape[0], d0q.shape[0]) >= film_rows(2 * N)
    check(_field_geo_bwd_dir(C.byref(net), ptr(stream), ptr(scales), groups, N, ptr(g_sdf), ptr(g_cos), ptr(a0q), ptr(a1q), ptr(d1q), ptr(d0q),
                             ptr(dET), 0 if dET is None else ld(dET), ptr(gmax), stream_ptr()), "nsky_field_geo_bwd_dir")


def native_weighted_colsum_pair(X, nt, rows, out, bias=None, g_sdf=None, g_cos=None):
    """the pair form over a pair-native X: w(row) = g_sdf[row // 2] on even rows (bias: those only), g_cos[row // 2] on odd rows"""
    check(_native_wcolsum_pair(ptr(X), nt, rows, ptr(g_sdf), ptr(g_cos), ptr(out), ld(out) if out.dim() == 2 else out.shape[0], ptr(bias),
                               stream_ptr()), "nsky_native_weighted_colsum_pair")


def pair_native_to_rows(buf, N: int, width: int):
    """pair-native [ceil32(2 N), width] -> [2, N, width] (row-set major; tests)"""
    return film_native_to_rows(buf, 2 * N, width).reshape(N, 2, width).permute(1, 0, 2)


def quad_native_to_rows(buf, N: int, width: int):
    """quad-native [ceil32(4 N), width] -> [4, N, width] (row-set major; tests)"""
    return film_native_to_rows(buf, 4 * N, width).reshape(N, 4, width).permute(1, 0, 2)


def _ptr_array(ts, n):
    arr = (C.c_void_p * FILM_MAX_LAYERS)()
    for i in range(n):
        arr[i] = None if ts is None or ts[i] is None else ts[i].data_ptr()
    return arr


def film_keepless(hidden: int) -> str:
    """how the chain kernels of this width run when the weights take no gradient and the weight gradients' operands (y_save, dz_save,
    dpre_save) are not kept: "registers" -- y_save, dz_save and dpre_save are None, the hand-offs between layers never leave the
    wave -- or "buffers": dz_save is None, y_save cycles two ping-pong buffers and every dpre_save entry is one shared buffer"""
    return "registers" if hidden == 128 else "buffers"


def film_saved_operands(hidden: int) -> bool:
    """whether the chain of this width keeps f = 15 F + 30 and the sine argument of every FiLM layer in the forward (film_chain_fwd, f_save / arg_save)
    and reads them back in the backward (film_chain_bwd_film, the same lists) instead of re-forming F and phase from the last mapping activation:
    two hidden x hidden products per layer less, 2 x 4 bytes per row and feature more written and read.  The default per width follows
    the same-box step measurement (profiles/film_saved_operands_ab.txt); NSKY_FILM_SAVED=0|1 overrides it for
    both widths, NSKY_FILM_SAVED=128 or 256 (comma-separated) names the widths that save"""
    env = os.environ.get("NSKY_FILM_SAVED", "")
    if env in ("0", "1"):
        return env == "1"
    if env:
        return str(hidden) in env.split(",")
    return hidden in FILM_SAVED_WIDTHS


def film_chain_fwd(net: FilmNet, stream_buf, scales, cond, x, M, h_save, z_save, y_save, res, f_save=None, arg_save=None):
    """see include/neusky_hip.h; h_save / z_save: lists (entries may be None) or None; y_save: list of [M, hidden] tensors, or None
    (film_keepless(hidden) == "registers"); f_save / arg_save: both None, or lists of tile-native [ceil32(M), hidden] tensors that take
    f = 15 F + 30 and the sine argument of every FiLM layer (nsky_film_chain_fwd_saved: the operands of film_chain_bwd_film's saved form)"""
    if f_save is not None or arg_save is not None:
        check(_film_fwd_saved(C.byref(net), ptr(stream_buf), ptr(scales), ptr(cond), ld(cond), ptr(x), ld(x), M,
                              _ptr_array(h_save, net.n_map), _ptr_array(z_save, net.n_film), _ptr_array(y_save, net.n_film),
                              _ptr_array(f_save, net.n_film), _ptr_array(arg_save, net.n_film), ptr(res), ld(res), stream_ptr()),
              "nsky_film_chain_fwd_saved")
        return res
    check(_film_fwd(C.byref(net), ptr(stream_buf), ptr(scales), ptr(cond), ld(cond), ptr(x), ld(x), M,
                    _ptr_array(h_save, net.n_map), _ptr_array(z_save, net.n_film), _ptr_array(y_save, net.n_film), ptr(res), ld(res),
                    stream_ptr()), "nsky_film_chain_fwd")
    return res


def film_rows(M: int) -> int:
    """rows of a tile-native activation matrix holding M batch rows"""
    return (M + 31) // 32 * 32


def film_native_to_rows(buf, M: int, width: int):
    """tile-native [ceil32(M), width] -> row-major [M, width] (tests / fallbacks; torch ops)"""
    R = film_rows(M) // 32
    return buf.reshape(R, width // 32, 4, 2, 32, 4).permute(0, 4, 1, 2, 3, 5).reshape(R * 32, width)[:M]


def film_rows_to_native(x, width: int):
    """row-major [M, width] -> tile-native [ceil32(M), width] (zero padded rows)"""
    M = x.shape[0]
    R = film_rows(M) // 32
    full = x.new_zeros(R * 32, width)
    full[:M] = x[:, :width]
    return full.reshape(R, 32, width // 32, 4, 2, 4).permute(0, 2, 3, 4, 1, 5).contiguous().reshape(R * 32, width)


def film_chain_bwd_film(net: FilmNet, stream_buf, table, M, d_res, h_last, z_save, dz_save, dfp, dfp_rowmax, gmax, d_x=None, f_save=None,
                        arg_save=None):
    """gmax: zero-filled float tensor [n_film + 1]; d_x: optional [M, ldx] output; dz_save: None = not kept (frozen weights; only
    gmax[n_film] is written); see include/neusky_hip.h.  f_save / arg_save (both, from film_chain_fwd): the saved-operand form
    (nsky_film_chain_bwd_film_saved) -- stream_buf / table packed with direction 3, h_last is not read and may be None"""
    if f_save is not None or arg_save is not None:
        check(_film_bwd_film_saved(C.byref(net), ptr(stream_buf), ptr(table), M, ptr(d_res), ld(d_res), _ptr_array(z_save, net.n_film),
                                   _ptr_array(f_save, net.n_film), _ptr_array(arg_save, net.n_film), _ptr_array(dz_save, net.n_film),
                                   ptr(dfp), ptr(dfp_rowmax), ptr(gmax), ptr(d_x), ld(d_x) if d_x is not None else 0, stream_ptr()),
              "nsky_film_chain_bwd_film_saved")
        return
    check(_film_bwd_film(C.byref(net), ptr(stream_buf), ptr(table), M, ptr(d_res), ld(d_res), ptr(h_last), _ptr_array(z_save, net.n_film),
                         _ptr_array(dz_save, net.n_film), ptr(dfp), ptr(dfp_rowmax), ptr(gmax), ptr(d_x), ld(d_x) if d_x is not None else 0,
                         stream_ptr()), "nsky_film_chain_bwd_film")


def film_chain_bwd_map(net: FilmNet, stream_buf, table, M, dfp, dfp_rowmax, h_save, dpre_save, d_cond, gmax):
    """gmax: zero-filled float tensor [n_map]; dpre_save: None (film_keepless(hidden) == "registers") or one shared buffer in every
    entry = not kept (frozen weights; gmax is not written)"""
    check(_film_bwd_map(C.byref(net), ptr(stream_buf), ptr(table), M, ptr(dfp), ptr(dfp_rowmax), _ptr_array(h_save, net.n_map),
                        _ptr_array(dpre_save, net.n_map), ptr(d_cond), ld(d_cond) if d_cond is not None else 0, ptr(gmax), stream_ptr()),
          "nsky_film_chain_bwd_map")


# ---- marching cubes (exporter/marching_cubes.py drives the three passes)
MC_TILE = 256  # NSKY_MC_TILE
_mc_count = _sig("nsky_mc_count", C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p)
_mc_vertices = _sig("nsky_mc_vertices", C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float,
                    C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_mc_faces = _sig("nsky_mc_faces", C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p)


def mc_count(volume, level: float, tile_counts):
    """volume: contiguous fp32 [nx, ny, nz]; tile_counts: int32 [4, ceil(nx ny nz / MC_TILE)] <- rows (vertices, faces, non-finite, 0)"""
    nx, ny, nz = volume.shape
    check(_mc_count(ptr(volume), nx, ny, nz, level, ptr(tile_counts), stream_ptr()), "nsky_mc_count")


def mc_vertices(volume, level: float, box_min, box_max, tile_vertex_offsets, base, edge_mask, vertices):
    """tile_vertex_offsets: int64 [n_tiles] exclusive scan; base: int32 [nx ny nz]; edge_mask: uint8 [nx ny nz]; vertices: fp32 [V, 3]"""
    nx, ny, nz = volume.shape
    check(_mc_vertices(ptr(volume), nx, ny, nz, level, *[float(v) for v in box_min], *[float(v) for v in box_max], ptr(tile_vertex_offsets),
                       ptr(base), ptr(edge_mask), ptr(vertices), stream_ptr()), "nsky_mc_vertices")


def mc_faces(volume, level: float, tile_face_offsets, base, edge_mask, faces):
    """tile_face_offsets: int64 [n_tiles] exclusive scan; faces: int32 [F, 3]"""
    nx, ny, nz = volume.shape
    check(_mc_faces(ptr(volume), nx, ny, nz, level, ptr(tile_face_offsets), ptr(base), ptr(edge_mask), ptr(faces), stream_ptr()),
          "nsky_mc_faces")


# ---- mesh simplification by vertex clustering (exporter/simplify.py drives keys -> sort -> reduce -> solve, remap -> sort -> compact)
MESH_KEY_BITS = 21  # NSKY_MESH_KEY_BITS
MESH_CELL_SUMS = 20  # NSKY_MESH_CELL_SUMS
_GRID = (C.c_double, C.c_double, C.c_double, C.c_double)
_mesh_cell_keys = _sig("nsky_mesh_cell_keys", C.c_void_p, C.c_int64, *_GRID, C.c_void_p, C.c_void_p)
_mesh_cluster_count = _sig("nsky_mesh_cluster_count", C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, *_GRID, C.c_void_p, C.c_void_p)
_mesh_vertex_cells = _sig("nsky_mesh_vertex_cells", C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
_mesh_remap_faces = _sig("nsky_mesh_remap_faces", C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_mesh_cluster_reduce = _sig("nsky_mesh_cluster_reduce", C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, *_GRID,
                            C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_mesh_cluster_solve = _sig("nsky_mesh_cluster_solve", C.c_void_p, C.c_void_p, C.c_int64, *_GRID, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p)
_mesh_flag_duplicates = _sig("nsky_mesh_flag_duplicates", C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_mesh_compact_faces = _sig("nsky_mesh_compact_faces", C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)


def _mesh_grid(lo, h):
    return [float(lo[0]), float(lo[1]), float(lo[2]), float(h)]


def _typed(t, dtype, *shape):
    """a contiguous tensor of this dtype and shape (None passes): what the mesh entry points index without a stride argument"""
    if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()):
        raise ValueError(f"expected a contiguous {dtype} tensor shaped {shape}, got {t.dtype} {tuple(t.shape)}")
    return t


def mesh_cell_keys(vertices, lo, h: float, keys):
    """vertices: fp32 [V, 3]; keys: int64 [V] <- the cell key of every vertex"""
    V = vertices.shape[0]
    check(_mesh_cell_keys(ptr(_typed(vertices, torch.float32, V, 3)), V, *_mesh_grid(lo, h), ptr(_typed(keys, torch.int64, V)), stream_ptr()),
          "nsky_mesh_cell_keys")


def mesh_cluster_count(vertices, faces, lo, h: float, count):
    """count: int64 [1], zeroed by the caller, += the faces with corners in three different cells"""
    V, F = vertices.shape[0], faces.shape[0]
    check(_mesh_cluster_count(ptr(_typed(vertices, torch.float32, V, 3)), V, ptr(_typed(faces, torch.int32, F, 3)), F, *_mesh_grid(lo, h),
                              ptr(_typed(count, torch.int64, 1)), stream_ptr()), "nsky_mesh_cluster_count")


def mesh_vertex_cells(vertex_order, rank_sorted, vertex_cell):
    """vertex_order, rank_sorted: int64 [V] (stable sort of the keys; rank of each sorted entry's cell); vertex_cell: int32 [V]"""
    V = vertex_order.shape[0]
    check(_mesh_vertex_cells(ptr(_typed(vertex_order, torch.int64, V)), ptr(_typed(rank_sorted, torch.int64, V)), V,
                             ptr(_typed(vertex_cell, torch.int32, V)), stream_ptr()), "nsky_mesh_vertex_cells")


def mesh_remap_faces(faces, vertex_cell, corner_cells, face_keys):
    """faces: int32 [F, 3]; vertex_cell: int32 [V]; corner_cells: int32 [F, 3]; face_keys: int64 [F]"""
    F, V = faces.shape[0], vertex_cell.shape[0]
    check(_mesh_remap_faces(ptr(_typed(faces, torch.int32, F, 3)), F, ptr(_typed(vertex_cell, torch.int32, V)), V,
                            ptr(_typed(corner_cells, torch.int32, F, 3)), ptr(_typed(face_keys, torch.int64, F)), stream_ptr()),
          "nsky_mesh_remap_faces")


def mesh_cluster_reduce(vertices, faces, normals, colours, lo, h: float, vertex_order, cell_start, sorted_corner_cells, corner_order,
                        cell_sums, group: int = 0):
    """cell_start: int64 [C + 1]; sorted_corner_cells: int32 [3 F], corner_order: int64 [3 F]; cell_sums: fp64 [C, MESH_CELL_SUMS];
    normals fp32 [V, 3] / colours uint8 [V, 3] or None; group: lanes per cell (0: chosen from the mean cell size, 8 or 64)"""
    V, F, Cn = vertices.shape[0], faces.shape[0], cell_sums.shape[0]
    check(_mesh_cluster_reduce(ptr(_typed(vertices, torch.float32, V, 3)), V, ptr(_typed(faces, torch.int32, F, 3)), F,
                               ptr(_typed(normals, torch.float32, V, 3)), ptr(_typed(colours, torch.uint8, V, 3)), *_mesh_grid(lo, h),
                               ptr(_typed(vertex_order, torch.int64, V)), ptr(_typed(cell_start, torch.int64, Cn + 1)), Cn,
                               ptr(_typed(sorted_corner_cells, torch.int32, 3 * F)), ptr(_typed(corner_order, torch.int64, 3 * F)), group,
                               ptr(_typed(cell_sums, torch.float64, Cn, MESH_CELL_SUMS)), stream_ptr()), "nsky_mesh_cluster_reduce")


def mesh_cluster_solve(cell_sums, cell_keys, lo, h: float, vertices_out, normals_out=None, colours_out=None):
    """cell_sums: fp64 [C, MESH_CELL_SUMS]; cell_keys: int64 [C] -> vertices_out fp32 [C, 3], normals_out fp32 / colours_out uint8 [C, 3]"""
    Cn = cell_sums.shape[0]
    check(_mesh_cluster_solve(ptr(_typed(cell_sums, torch.float64, Cn, MESH_CELL_SUMS)), ptr(_typed(cell_keys, torch.int64, Cn)), Cn,
                              *_mesh_grid(lo, h), ptr(_typed(vertices_out, torch.float32, Cn, 3)), ptr(_typed(normals_out, torch.float32, Cn, 3)),
                              ptr(_typed(colours_out, torch.uint8, Cn, 3)), stream_ptr()), "nsky_mesh_cluster_solve")


def mesh_flag_duplicates(corner_cells, sorted_keys, face_order, keep):
    """sorted_keys, face_order: int64 [F] (stable sort of the face keys); keep: int32 [F] <- 1 for a face that stays"""
    F = corner_cells.shape[0]
    check(_mesh_flag_duplicates(ptr(_typed(corner_cells, torch.int32, F, 3)), F, ptr(_typed(sorted_keys, torch.int64, F)),
                                ptr(_typed(face_order, torch.int64, F)), ptr(_typed(keep, torch.int32, F)), stream_ptr()),
          "nsky_mesh_flag_duplicates")


def mesh_compact_faces(corner_cells, keep, ends, faces_out):
    """ends: int64 [F], the inclusive scan of keep; faces_out: int32 [ends[-1], 3]"""
    F, Fo = corner_cells.shape[0], faces_out.shape[0]
    check(_mesh_compact_faces(ptr(_typed(corner_cells, torch.int32, F, 3)), F, ptr(_typed(keep, torch.int32, F)), ptr(_typed(ends, torch.int64, F)),
                              Fo, ptr(_typed(faces_out, torch.int32, Fo, 3)), stream_ptr()), "nsky_mesh_compact_faces")


# ---- connected components of a mesh (exporter/components.py drives link -> flatten -> rank (torch) -> select -> scan (torch) -> compact)
CC_STATUS_INDEX, CC_STATUS_LINK, CC_STATUS_FLATTEN = 1, 2, 4  # NSKY_CC_STATUS_*
_cc_link = _sig("nsky_cc_link", C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_cc_flatten = _sig("nsky_cc_flatten", C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_cc_select = _sig("nsky_cc_select", C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_cc_compact = _sig("nsky_cc_compact", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                   C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def cc_link(faces, parent, status):
    """faces: int32 [F, 3]; parent: int32 [V], the identity on entry, a forest on return; status: int32 [1], zeroed by the caller"""
    F, V = faces.shape[0], parent.shape[0]
    check(_cc_link(ptr(_typed(faces, torch.int32, F, 3)), F, V, ptr(_typed(parent, torch.int32, V)), ptr(_typed(status, torch.int32, 1)),
                   stream_ptr()), "nsky_cc_link")


def cc_flatten(parent, faces, vertex_root, face_root, status):
    """parent: int32 [V] after cc_link -> vertex_root: int32 [V], face_root: int32 [F] (the root of the first corner)"""
    F, V = faces.shape[0], parent.shape[0]
    check(_cc_flatten(ptr(_typed(parent, torch.int32, V)), V, ptr(_typed(faces, torch.int32, F, 3)), F, ptr(_typed(vertex_root, torch.int32, V)),
                      ptr(_typed(face_root, torch.int32, F)), ptr(_typed(status, torch.int32, 1)), stream_ptr()), "nsky_cc_flatten")


def cc_select(faces, face_labels, keep_component, keep, vertex_used):
    """face_labels: int32 [F]; keep_component: uint8 [C] -> keep: uint8 [F]; vertex_used: uint8 [V], zeroed by the caller"""
    F, V, Cn = faces.shape[0], vertex_used.shape[0], keep_component.shape[0]
    check(_cc_select(ptr(_typed(faces, torch.int32, F, 3)), F, V, ptr(_typed(face_labels, torch.int32, F)),
                     ptr(_typed(keep_component, torch.uint8, Cn)), Cn, ptr(_typed(keep, torch.uint8, F)),
                     ptr(_typed(vertex_used, torch.uint8, V)), stream_ptr()), "nsky_cc_select")


def cc_compact(vertices, normals, colours, faces, keep, face_ends, vertex_used, vertex_ends, vertices_out, normals_out, colours_out, faces_out):
    """face_ends: int64 [F] / vertex_ends: int64 [V], the inclusive scans of keep / vertex_used; the outputs are sized by their last
    entries; normals fp32 [V, 3] / colours uint8 [V, 3] or None, each with its output"""
    V, F, Vo, Fo = vertices.shape[0], faces.shape[0], vertices_out.shape[0], faces_out.shape[0]
    check(_cc_compact(ptr(_typed(vertices, torch.float32, V, 3)), ptr(_typed(normals, torch.float32, V, 3)), ptr(_typed(colours, torch.uint8, V, 3)),
                      V, ptr(_typed(faces, torch.int32, F, 3)), F, ptr(_typed(keep, torch.uint8, F)), ptr(_typed(face_ends, torch.int64, F)),
                      ptr(_typed(vertex_used, torch.uint8, V)), ptr(_typed(vertex_ends, torch.int64, V)), Vo, Fo,
                      ptr(_typed(vertices_out, torch.float32, Vo, 3)), ptr(_typed(normals_out, torch.float32, Vo, 3)),
                      ptr(_typed(colours_out, torch.uint8, Vo, 3)), ptr(_typed(faces_out, torch.int32, Fo, 3)), stream_ptr()), "nsky_cc_compact")


# ---- texture baking on a per-triangle-pair atlas (exporter/texture.py drives texel points -> the field's value chain -> texel store)
TEXTURE_MAX_SIZE = 16384  # NSKY_TEXTURE_MAX_SIZE
_texture_texel_points = _sig("nsky_texture_texel_points", C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                             C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_texture_texel_store = _sig("nsky_texture_texel_store", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                            C.c_void_p, C.c_void_p)


def texture_texel_points(vertices, faces, px_per_uv_triangle: int, squares_per_row: int, s0: int, s1: int, owner, offset, points):
    """vertices: fp32 [V, 3]; faces: int32 [F, 3]; the n = (s1 - s0) (P + 3)^2 texels of squares [s0, s1) -> owner: int32 [n] (-1: none),
    offset: int64 [n] (y W + x), points: fp32 [n, 3]"""
    V, F = vertices.shape[0], faces.shape[0]
    n = (int(s1) - int(s0)) * (int(px_per_uv_triangle) + 3) ** 2
    check(_texture_texel_points(ptr(_typed(vertices, torch.float32, V, 3)), V, ptr(_typed(faces, torch.int32, F, 3)), F, int(px_per_uv_triangle),
                                int(squares_per_row), int(s0), int(s1), ptr(_typed(owner, torch.int32, n)), ptr(_typed(offset, torch.int64, n)),
                                ptr(_typed(points, torch.float32, n, 3)), stream_ptr()), "nsky_texture_texel_points")


def texture_texel_store(albedo, gradient, owner, offset, image, normal_image=None):
    """albedo (linear), gradient: fp32 [n, 3] (gradient may be None without a normal image); owner: int32 [n]; offset: int64 [n];
    image, normal_image: uint8 [W, W, 3], written at the offsets of the owned texels"""
    n, W = owner.shape[0], image.shape[0]
    check(_texture_texel_store(ptr(_typed(albedo, torch.float32, n, 3)), ptr(_typed(gradient, torch.float32, n, 3)),
                               ptr(_typed(owner, torch.int32, n)), ptr(_typed(offset, torch.int64, n)), n, W,
                               ptr(_typed(image, torch.uint8, W, W, 3)), ptr(_typed(normal_image, torch.uint8, W, W, 3)), stream_ptr()),
          "nsky_texture_texel_store")


# ---- environment-map relighting (relight/envmap.py drives label -> stable sort -> reduce, and the lookup)
ENVMAP_NEUSKY, ENVMAP_BLENDER = 0, 1  # NSKY_ENVMAP_NEUSKY / _BLENDER
ENVMAP_MAX_DIRECTIONS = 1024  # NSKY_ENVMAP_MAX_DIRECTIONS
_envmap_label = _sig("nsky_envmap_label", C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p)
_envmap_reduce = _sig("nsky_envmap_reduce", C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_envmap_lookup = _sig("nsky_envmap_lookup", C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                      C.c_void_p, C.c_void_p)


def envmap_label(directions, rotation, H: int, W: int, convention: int, labels):
    """directions: fp32 [D, 3]; rotation: fp32 [3, 3] or None; labels: int16 [H W] <- the cell of every texel"""
    check(_envmap_label(ptr(directions), directions.shape[0], ptr(rotation), H, W, convention, ptr(labels), stream_ptr()), "nsky_envmap_label")


def envmap_reduce(data, convention: int, directions, rotation, exposure, sorted_labels, order, colours, cell_weight):
    """data: fp32 [H, W, 3]; exposure: fp32 [1] or None; sorted_labels int16 / order int64 [H W] (stable sort of the labels);
    colours: fp32 [D, 3], cell_weight: fp32 [D]"""
    H, W = data.shape[:2]
    check(_envmap_reduce(ptr(data), H, W, convention, ptr(directions), directions.shape[0], ptr(rotation), ptr(exposure), ptr(sorted_labels),
                         ptr(order), ptr(colours), ptr(cell_weight), stream_ptr()), "nsky_envmap_reduce")


def envmap_lookup(data, convention: int, directions, rotation, exposure, out):
    """data: fp32 [H, W, 3]; directions: fp32 [N, 3]; out: fp32 [N, 3]"""
    H, W = data.shape[:2]
    check(_envmap_lookup(ptr(data), H, W, convention, ptr(directions), directions.shape[0], ptr(rotation), ptr(exposure), ptr(out),
                         stream_ptr()), "nsky_envmap_lookup")


# ---- the sun of an environment map (relight/envmap_sun.py, csrc/envmap_sun.hip): peak -> ring -> split on one stream, no host reads
ENVMAP_SUN_SCRATCH_BYTES = 1024 * 7 * 8  # NSKY_ENVMAP_SUN_SCRATCH_BYTES
_envmap_peak = _sig("nsky_envmap_peak", C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_envmap_sun_ring = _sig("nsky_envmap_sun_ring", C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                        C.c_void_p)
_envmap_sun_split = _sig("nsky_envmap_sun_split", C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def _envmap_sun_map(data, scratch):
    H, W = data.shape[:2]
    _typed(data, torch.float32, H, W, 3)
    _typed(scratch, torch.float64, ENVMAP_SUN_SCRATCH_BYTES // 8)
    return H, W


def envmap_peak(data, convention: int, scratch, peak):
    """data: fp32 [H, W, 3]; scratch: fp64 [ENVMAP_SUN_SCRATCH_BYTES / 8]; peak: int64 [2] <- the texel index, then the bits of the fp64
    luminance (peak.view(torch.float64)[1])"""
    H, W = _envmap_sun_map(data, scratch)
    check(_envmap_peak(ptr(data), H, W, convention, ptr(scratch), ptr(_typed(peak, torch.int64, 2)), stream_ptr()), "nsky_envmap_peak")


def envmap_sun_ring(data, convention: int, peak, rho: float, scratch, ring):
    """peak: as envmap_peak left it; rho: radians; ring: fp64 [2] <- sum omega, sum omega Y over the annulus [rho, 2 rho) about the peak"""
    H, W = _envmap_sun_map(data, scratch)
    check(_envmap_sun_ring(ptr(data), H, W, convention, ptr(_typed(peak, torch.int64, 2)), float(rho), ptr(scratch),
                           ptr(_typed(ring, torch.float64, 2)), stream_ptr()), "nsky_envmap_sun_ring")


def envmap_sun_split(data, convention: int, peak, ring, rho: float, min_peak_ratio: float, scratch, residual, stats):
    """residual: fp32 [H, W, 3] <- the map without its sun; stats: fp64 [12] <- m (3), C (3), Y_p, tau, Omega_sun, found, peak row, column"""
    H, W = _envmap_sun_map(data, scratch)
    check(_envmap_sun_split(ptr(data), H, W, convention, ptr(_typed(peak, torch.int64, 2)), ptr(_typed(ring, torch.float64, 2)), float(rho),
                            float(min_peak_ratio), ptr(scratch), ptr(_typed(residual, torch.float32, H, W, 3)),
                            ptr(_typed(stats, torch.float64, 12)), stream_ptr()), "nsky_envmap_sun_split")


# ---- precomputed radiance transfer (relight/transfer.py): bake a frame's light-independent part once, relight it per light
TRANSFER_FP32, TRANSFER_FP16 = 0, 1  # NSKY_TRANSFER_FP32 / _FP16
TRANSFER_MAX_DIRECTIONS = 1024  # NSKY_TRANSFER_MAX_DIRECTIONS
_transfer_bake = _sig("nsky_transfer_bake", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                      C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)
_transfer_relight = _sig("nsky_transfer_relight", C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)


def _transfer_storage(T, exponents) -> int:
    if T.dtype == torch.float32:
        return TRANSFER_FP32
    if T.dtype != torch.float16:
        raise ValueError(f"a transfer is stored as float32 or float16, not {T.dtype}")
    if exponents is None or exponents.dtype != torch.int32:
        raise ValueError("float16 transfer storage needs its int32 row exponents")
    return TRANSFER_FP16


def _ray_samples(albedo, normals, weights, positions=None):
    """(R, S) of the samples along a batch of rays: albedo, normals and, if given, positions fp32 [R, S, 3]; weights fp32 [R, S]"""
    R, S, _ = albedo.shape
    assert albedo.shape == (R, S, 3) and normals.shape == (R, S, 3) and weights.shape == (R, S)
    assert positions is None or positions.shape == (R, S, 3)
    assert all(t is None or t.dtype == torch.float32 for t in (albedo, normals, weights, positions))
    return R, S


def _relight_operands(rows, exponents, acc, lights, bg, rgb, lin):
    """(R, n, K, storage) of a relight: rows fp32 or fp16 [R, n, 3] (+ exponents int32 [R]); acc fp32 [R]; lights fp32 [K, n, 3]; bg, rgb
    and, if given, lin fp32 [K, R, 3]"""
    R, n, _ = rows.shape
    K = lights.shape[0]
    assert lights.shape == (K, n, 3) and bg.shape == (K, R, 3) and rgb.shape == (K, R, 3) and acc.shape[0] == R
    assert lin is None or lin.shape == (K, R, 3)
    assert all(t.dtype == torch.float32 for t in (acc, lights, bg, rgb)) and (lin is None or lin.dtype == torch.float32)
    assert exponents is None or exponents.shape[0] == R
    return R, n, K, _transfer_storage(rows, exponents)


def transfer_bake(albedo, normals, weights, dirs, vis, T, row0: int, exponents, acc):
    """albedo, normals: fp32 [R, S, 3]; weights [R, S]; dirs [D, 3]; vis [R, D] or None -> rows [row0, row0 + R) of T (fp32 or fp16
    [rows, D, 3]), exponents: int32 [R] (fp16 storage, else None), acc: fp32 [R]"""
    R, S = _ray_samples(albedo, normals, weights)
    D = dirs.shape[0]
    if T.dim() != 3 or tuple(T.shape[1:]) != (D, 3) or not 0 <= row0 <= T.shape[0] - R:
        raise ValueError(f"rows [{row0}, {row0 + R}) of a transfer shaped {tuple(T.shape)} for D = {D}")
    assert acc.shape[0] == R and (vis is None or vis.shape == (R, D))
    assert exponents is None or exponents.shape[0] == R
    check(_transfer_bake(_c(albedo), _c(normals), _c(weights), _c(dirs), _c(vis), R, S, D, _transfer_storage(T, exponents), _c(T), row0,
                         _c(exponents), _c(acc), stream_ptr()), "nsky_transfer_bake")


def transfer_relight(T, exponents, acc, lights, bg, rgb, lin=None):
    """T: fp32 or fp16 [R, D, 3] (+ exponents int32 [R]); acc: fp32 [R]; lights: fp32 [K, D, 3]; bg: fp32 [K, R, 3] -> rgb [K, R, 3]
    (sRGB, clamped) and, if given, lin [K, R, 3]"""
    R, D, K, storage = _relight_operands(T, exponents, acc, lights, bg, rgb, lin)
    check(_transfer_relight(_c(T), storage, _c(exponents), _c(acc), _c(lights), _c(bg), R, D, K, _c(rgb), _c(lin), stream_ptr()),
          "nsky_transfer_relight")


# ---- a radiance transfer in a basis of the light directions (relight/transfer_sh.py, csrc/transfer_sh.hip)
TRANSFER_MAX_COEFFICIENTS = 128  # NSKY_TRANSFER_MAX_COEFFICIENTS
_transfer_project = _sig("nsky_transfer_project", C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
_transfer_relight_short = _sig("nsky_transfer_relight_short", C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)


def transfer_project(T, exponents, basis, coeffs, row0: int = 0, coeff_exponents=None):
    """T: fp32 or fp16 [R, D, 3] (+ exponents int32 [R]); basis: fp32 [D, J] -> rows [row0, row0 + R) of coeffs (fp32 or fp16
    [rows, J, 3]) and, for fp16, of coeff_exponents (int32 [rows]): coeffs[row0 + r, j, c] = sum_d T[r, d, c] basis[d, j]"""
    R, D, _ = T.shape
    J = basis.shape[1]
    if not 1 <= J <= TRANSFER_MAX_COEFFICIENTS or not 1 <= D <= TRANSFER_MAX_DIRECTIONS:
        raise ValueError(f"a projection takes 1..{TRANSFER_MAX_DIRECTIONS} directions onto 1..{TRANSFER_MAX_COEFFICIENTS} coefficients, not "
                         f"{D} onto {J}")
    if coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (J, 3) or not 0 <= row0 <= coeffs.shape[0] - R:
        raise ValueError(f"rows [{row0}, {row0 + R}) of coefficients shaped {tuple(coeffs.shape)} for J = {J}")
    assert T.shape[2] == 3 and basis.shape == (D, J) and basis.dtype == torch.float32
    assert exponents is None or exponents.shape[0] == R
    assert coeff_exponents is None or coeff_exponents.reshape(-1).shape[0] == coeffs.shape[0]
    check(_transfer_project(_c(T), _transfer_storage(T, exponents), _c(exponents), _c(basis), R, D, J,
                            _transfer_storage(coeffs, coeff_exponents), _c(coeffs), row0, _c(coeff_exponents), stream_ptr()),
          "nsky_transfer_project")


def transfer_relight_short(coeffs, exponents, acc, lights, bg, rgb, lin=None):
    """transfer_relight for rows of coefficients: coeffs: fp32 or fp16 [R, J, 3] (+ exponents int32 [R]), any J in 1..128; lights: fp32
    [K, J, 3]; bg: fp32 [K, R, 3] -> rgb [K, R, 3] (sRGB, clamped) and, if given, lin [K, R, 3]"""
    if not 1 <= coeffs.shape[1] <= TRANSFER_MAX_COEFFICIENTS:
        raise ValueError(f"rows of 1..{TRANSFER_MAX_COEFFICIENTS} coefficients, not {coeffs.shape[1]}")
    R, J, K, storage = _relight_operands(coeffs, exponents, acc, lights, bg, rgb, lin)
    check(_transfer_relight_short(_c(coeffs), storage, _c(exponents), _c(acc), _c(lights), _c(bg), R, J, K, _c(rgb), _c(lin), stream_ptr()),
          "nsky_transfer_relight_short")


# ---- a directional sun on top of the hemisphere render (relight/sun.py, csrc/sun.hip)
_sun_transfer = _sig("nsky_sun_transfer", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                     C.c_void_p)
_sun_composite = _sig("nsky_sun_composite", C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def sun_transfer(albedo, normals, weights, suns, out):
    """albedo, normals: fp32 [R, S, 3]; weights [R, S]; suns [K, 3] -> out [K, R, 3]"""
    R, S = _ray_samples(albedo, normals, weights)
    K = suns.shape[0]
    assert suns.shape == (K, 3) and out.shape == (K, R, 3) and suns.dtype == torch.float32 and out.dtype == torch.float32
    check(_sun_transfer(_c(albedo), _c(normals), _c(weights), _c(suns), R, S, K, _c(out), stream_ptr()), "nsky_sun_transfer")


def sun_composite(lin_sky, t, vis, acc, acc_threshold, suns, colours, rgb, lin=None, shadow=None):
    """lin_sky: fp32 [R, 3] (one sky under all K suns) or [K, R, 3] (a sky of each sun's own); t [K, R, 3]; vis [K, R] or None; acc [R];
    acc_threshold [1] (device); suns, colours [K, 3] -> rgb [K, R, 3] (sRGB, clamped) and, if given, lin [K, R, 3] and shadow [K, R]"""
    K, R, _ = t.shape
    assert lin_sky.shape in ((R, 3), (K, R, 3)) and acc.numel() == R and acc_threshold.numel() == 1 and suns.shape == (K, 3) and colours.shape == (K, 3)
    assert rgb.shape == (K, R, 3) and (vis is None or vis.shape == (K, R)) and (lin is None or lin.shape == (K, R, 3))
    assert shadow is None or shadow.shape == (K, R)
    assert all(x is None or x.dtype == torch.float32 for x in (lin_sky, t, vis, acc, acc_threshold, suns, colours, rgb, lin, shadow))
    stride = 0 if lin_sky.dim() == 2 else R * 3
    check(_sun_composite(_c(lin_sky), stride, _c(t), _c(vis), _c(acc), _c(acc_threshold), _c(suns), _c(colours), R, K, _c(rgb), _c(lin),
                         _c(shadow), stream_ptr()), "nsky_sun_composite")


# ---- a clear-sky daylight model whose sky follows the sun (relight/daylight.py, csrc/daylight.hip)
_daylight_eval = _sig("nsky_daylight_eval", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                      C.c_void_p)


def daylight_eval(directions, suns, turbidity, exposure, ground, out):
    """directions: fp32 [N, 3]; suns [K, 3]; turbidity, exposure [1], ground [3] (device) -> out [K, N, 3]"""
    N, K = directions.shape[0], suns.shape[0]
    assert directions.shape == (N, 3) and suns.shape == (K, 3) and out.shape == (K, N, 3) and N >= 1 and K >= 1
    assert turbidity.numel() == 1 and exposure.numel() == 1 and ground.numel() == 3
    assert all(x.dtype == torch.float32 for x in (directions, suns, turbidity, exposure, ground, out))
    check(_daylight_eval(_c(directions), _c(suns), _c(turbidity), _c(exposure), _c(ground), N, K, _c(out), stream_ptr()), "nsky_daylight_eval")


# ---- sphere-traced shadow rays through the SDF (relight/shadows.py, csrc/sphere_trace.hip)
TRACE_ALIVE, TRACE_HIT, TRACE_ESCAPED, TRACE_EXHAUSTED = 0, 1, 2, 3
TRACE_PARAMS = 6  # eps, relax, min_step, tan_half, radius, bias
_sphere_trace_begin = _sig("nsky_sphere_trace_begin", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_sphere_trace_begin_points = _sig("nsky_sphere_trace_begin_points", C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p)
_sphere_trace_step = _sig("nsky_sphere_trace_step", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                          C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)
_sphere_trace_finish = _sig("nsky_sphere_trace_finish", C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def _trace_buffers(T, params, state, points, ray_dirs=None, bounds=None):
    """the buffers of a march of T rays; with ray_dirs [T, 3] and bounds [2, T] (t_end, tan_half): of rays that end at a light"""
    assert params.shape == (TRACE_PARAMS,) and state.shape == (6, T) and points.shape == (T, 3)
    assert (ray_dirs is None) == (bounds is None) and (bounds is None or (ray_dirs.shape == (T, 3) and bounds.shape == (2, T)))
    assert all(x is None or (x.dtype == torch.float32 and x.is_contiguous()) for x in (params, state, points, ray_dirs, bounds))


def sphere_trace_begin(origins, directions, depth, normals, suns, params, state, points):
    """origins, directions, normals: fp32 [R, 3]; depth [R]; suns [K, 3]; params [6] (device) -> state [6, K R], points [K R, 3]"""
    R, K = origins.shape[0], suns.shape[0]
    assert origins.shape == (R, 3) and directions.shape == (R, 3) and normals.shape == (R, 3) and depth.numel() == R and suns.shape == (K, 3)
    assert all(x.dtype == torch.float32 for x in (origins, directions, depth, normals, suns))
    _trace_buffers(K * R, params, state, points)
    check(_sphere_trace_begin(_c(origins), _c(directions), _c(depth), _c(normals), _c(suns), R, K, ptr(params), ptr(state), ptr(points),
                              stream_ptr()), "nsky_sphere_trace_begin")


def sphere_trace_begin_points(starts, directions, params, state, points):
    """starts: fp32 [M, 3]; directions [M, 3] (one per ray) or [K, 3] (every start under every direction, ray k M + r) -> state, points"""
    M, T = starts.shape[0], points.shape[0]
    assert starts.shape == (M, 3) and directions.dim() == 2 and directions.shape[1] == 3 and M >= 1
    assert starts.dtype == torch.float32 and directions.dtype == torch.float32
    dir_div = trace_dir_div(directions, M, T)
    _trace_buffers(T, params, state, points)
    check(_sphere_trace_begin_points(_c(starts), _c(directions), M, T, dir_div, ptr(params), ptr(state), ptr(points), stream_ptr()),
          "nsky_sphere_trace_begin_points")


def trace_dir_div(directions, M: int, T: int) -> int:
    """rays per direction row: 1 for a direction of each ray's own ([T, 3]), M for K directions over M starts (T = K M)"""
    if T == M and directions.shape[0] == M:
        return 1
    if directions.shape[0] * M != T:
        raise ValueError(f"{T} rays from {M} start points and {directions.shape[0]} directions")
    return M


def sphere_trace_step(state, sdf, directions, dir_div: int, params, iteration: int, steps: int, grace: int, points, bounds=None):
    """one round of the march: state [6, T], sdf fp32 [T] at `points`, directions [T / dir_div, 3] -> state, points [T, 3].  bounds
    [2, T] (t_end, tan_half): the round of rays that end at a light, each with a direction of its own (dir_div 1, directions [T, 3])"""
    T = points.shape[0]
    if bounds is not None and not (dir_div == 1 and directions.shape == (T, 3) and bounds.shape == (2, T)):
        raise NeuSkyHipError(f"sphere_trace_step: bounds [2, {T}] go with dir_div 1 and directions [{T}, 3], got bounds "
                             f"{tuple(bounds.shape)}, dir_div {dir_div}, directions {tuple(directions.shape)}")
    _trace_buffers(T, params, state, points, None if bounds is None else directions, bounds)
    assert sdf.dtype == torch.float32 and sdf.numel() == T and directions.dtype == torch.float32
    assert dir_div >= 1 and directions.shape == (-(-T // dir_div), 3) and 0 <= iteration < steps
    check(_sphere_trace_step(ptr(state), _c(sdf), _c(directions), ptr(bounds), T, dir_div, ptr(params), iteration, steps, grace, ptr(points),
                             stream_ptr()), "nsky_sphere_trace_step")


def sphere_trace_finish(state, vis, status, t):
    """state [6, T] -> vis, t: fp32 [T]; status: int8 [T]"""
    T = state.shape[1]
    assert state.shape == (6, T) and state.dtype == torch.float32 and state.is_contiguous()
    assert vis.numel() == T and t.numel() == T and status.numel() == T and status.dtype == torch.int8
    assert vis.dtype == torch.float32 and t.dtype == torch.float32 and all(x.is_contiguous() for x in (vis, status, t))
    check(_sphere_trace_finish(ptr(state), T, ptr(vis), ptr(status), ptr(t), stream_ptr()), "nsky_sphere_trace_finish")


# ---- point and spot lights inside the scene (relight/lights.py, csrc/lights.hip; their march: sphere_trace_step with bounds)
LIGHT_FLOATS = 16  # NSKY_LIGHT_FLOATS: p (0..2), a (3..5), cos_inner, cos_outer, rho, clearance, min_distance, -, I (12..14), -
_light_transfer = _sig("nsky_light_transfer", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                       C.c_void_p, C.c_void_p)
_light_trace_begin = _sig("nsky_light_trace_begin", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_light_trace_begin_points = _sig("nsky_light_trace_begin_points", C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_lights_composite = _sig("nsky_lights_composite", C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)


def _lights_block(lights):
    L = lights.shape[0]
    assert lights.shape == (L, LIGHT_FLOATS) and L >= 1 and lights.dtype == torch.float32 and lights.is_contiguous()
    return L


def light_transfer(positions, albedo, normals, weights, lights, out):
    """positions, albedo, normals: fp32 [R, S, 3]; weights [R, S]; lights [L, 16] -> out [L, R, 3]"""
    assert positions is not None
    R, S = _ray_samples(albedo, normals, weights, positions)
    L = _lights_block(lights)
    assert out.shape == (L, R, 3) and out.dtype == torch.float32
    check(_light_transfer(_c(positions), _c(albedo), _c(normals), _c(weights), ptr(lights), R, S, L, _c(out), stream_ptr()),
          "nsky_light_transfer")


def light_trace_begin(origins, directions, depth, normals, lights, params, state, points, ray_dirs, bounds):
    """origins, directions, normals: fp32 [R, 3]; depth [R]; lights [L, 16]; params [6] (device) -> state [6, L R], points, ray_dirs
    [L R, 3], bounds [2, L R] (t_end, tan_half)"""
    R, L = origins.shape[0], _lights_block(lights)
    assert origins.shape == (R, 3) and directions.shape == (R, 3) and normals.shape == (R, 3) and depth.numel() == R
    assert all(x.dtype == torch.float32 for x in (origins, directions, depth, normals))
    _trace_buffers(L * R, params, state, points, ray_dirs, bounds)
    check(_light_trace_begin(_c(origins), _c(directions), _c(depth), _c(normals), ptr(lights), R, L, ptr(params), ptr(state), ptr(points),
                             ptr(ray_dirs), ptr(bounds), stream_ptr()), "nsky_light_trace_begin")


def light_trace_begin_points(starts, lights, params, state, points, ray_dirs, bounds):
    """starts: fp32 [M, 3]; lights [L, 16] (every start under every light, ray l M + r) -> state, points, ray_dirs, bounds"""
    M, L = starts.shape[0], _lights_block(lights)
    assert starts.shape == (M, 3) and M >= 1 and starts.dtype == torch.float32
    _trace_buffers(L * M, params, state, points, ray_dirs, bounds)
    check(_light_trace_begin_points(_c(starts), ptr(lights), M, L, ptr(params), ptr(state), ptr(points), ptr(ray_dirs), ptr(bounds),
                                    stream_ptr()), "nsky_light_trace_begin_points")


def lights_composite(base, t, vis, acc, acc_threshold, lights, rgb, lin=None, light_lin=None, visibility=None):
    """base: fp32 [R, 3] (one base under all Kb outputs) or [Kb, R, 3]; t [L, R, 3]; vis [L, R] or None; acc [R]; acc_threshold [1]
    (device); lights [L, 16] -> rgb [Kb, R, 3] (sRGB, clamped) and, if given, lin [Kb, R, 3], light_lin [R, 3], visibility [L, R]"""
    L, R, _ = t.shape
    Kb = rgb.shape[0]
    assert _lights_block(lights) == L and rgb.shape == (Kb, R, 3) and base.shape in ((R, 3), (Kb, R, 3))
    assert acc.numel() == R and acc_threshold.numel() == 1 and (vis is None or vis.shape == (L, R)) and (lin is None or lin.shape == (Kb, R, 3))
    assert (light_lin is None or light_lin.shape == (R, 3)) and (visibility is None or visibility.shape == (L, R))
    assert all(x is None or x.dtype == torch.float32 for x in (base, t, vis, acc, acc_threshold, rgb, lin, light_lin, visibility))
    stride = 0 if base.dim() == 2 else R * 3
    check(_lights_composite(_c(base), stride, _c(t), _c(vis), _c(acc), _c(acc_threshold), ptr(lights), R, L, Kb, _c(rgb), _c(lin), _c(light_lin),
                            _c(visibility), stream_ptr()), "nsky_lights_composite")


# ---- solid props placed in a frame (relight/props.py, csrc/props.hip)
PROP_FLOATS = 16  # NSKY_PROP_FLOATS: kind, c (1..3), h (4..6), cos yaw, sin yaw, albedo (9..11), visible, casts_shadows, -, -
MAX_PROPS = 64  # NSKY_MAX_PROPS
_props_intersect = _sig("nsky_props_intersect", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p, C.c_void_p)
_props_insert = _sig("nsky_props_insert", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                     C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_props_occlude = _sig("nsky_props_occlude", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                      C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)


def _props_block(props):
    P = props.shape[0]
    assert props.shape == (P, PROP_FLOATS) and 1 <= P <= MAX_PROPS and props.dtype == torch.float32 and props.is_contiguous()
    return P


def props_intersect(origins, directions, props, t_hit, prop_id, normal, albedo):
    """origins, directions: fp32 [R, 3]; props [P, 16] -> t_hit [R] (+inf for none), prop_id int32 [R] (-1), normal, albedo [R, 3]"""
    R, P = origins.shape[0], _props_block(props)
    assert origins.shape == (R, 3) and directions.shape == (R, 3) and normal.shape == (R, 3) and albedo.shape == (R, 3)
    assert t_hit.shape == (R,) and prop_id.shape == (R,) and prop_id.dtype == torch.int32
    assert all(x.dtype == torch.float32 for x in (origins, directions, t_hit, normal, albedo))
    check(_props_intersect(_c(origins), _c(directions), ptr(props), R, P, _c(t_hit), _c(prop_id), _c(normal), _c(albedo), stream_ptr()),
          "nsky_props_intersect")


def props_insert(weights, starts, ends, albedo, normals, t_hit, prop_id, hit_normal, hit_albedo, weights_out, starts_out, ends_out, albedo_out,
                 normals_out):
    """weights, starts, ends: fp32 [R, S]; albedo, normals [R, S, 3]; the four outputs of props_intersect -> the five arrays with S + 1
    samples"""
    R, S = _ray_samples(albedo, normals, weights)
    assert S >= 1 and starts.shape == (R, S) and ends.shape == (R, S) and t_hit.shape == (R,) and prop_id.shape == (R,)
    assert hit_normal.shape == (R, 3) and hit_albedo.shape == (R, 3) and prop_id.dtype == torch.int32
    assert all(x.shape == (R, S + 1) for x in (weights_out, starts_out, ends_out)) and albedo_out.shape == (R, S + 1, 3)
    assert normals_out.shape == (R, S + 1, 3)
    assert all(x.dtype == torch.float32 for x in (starts, ends, t_hit, hit_normal, hit_albedo, weights_out, starts_out, ends_out, albedo_out,
                                                  normals_out))
    check(_props_insert(_c(weights), _c(starts), _c(ends), _c(albedo), _c(normals), _c(t_hit), _c(prop_id), _c(hit_normal), _c(hit_albedo), R, S,
                        _c(weights_out), _c(starts_out), _c(ends_out), _c(albedo_out), _c(normals_out), stream_ptr()), "nsky_props_insert")


def props_occlude(x, normals, bias, props, vis, directions=None, targets=None, clearance=None):
    """x: fp32 [M, 3]; normals [M, 3] or None; either directions [N, 3] (lights at infinity) or targets [N, 3] with clearance [N] (lamps);
    bias [1] (device); props [P, 16] -> vis: fp32 [M, N] through its strides (a transposed view of [N, M] serves), in place: 0 where a
    shadow-casting prop stands between point m and light n"""
    M, P = x.shape[0], _props_block(props)
    towards = directions if directions is not None else targets
    assert (directions is None) != (targets is None) and (targets is None) == (clearance is None)
    N = towards.shape[0]
    assert x.shape == (M, 3) and towards.shape == (N, 3) and (normals is None or normals.shape == (M, 3)) and bias.numel() == 1
    assert clearance is None or clearance.shape == (N,)
    assert all(t is None or t.dtype == torch.float32 for t in (x, normals, towards, clearance, bias, vis))
    if tuple(vis.shape) != (M, N):
        raise ValueError(f"vis: [{M}, {N}] (points, lights), got {tuple(vis.shape)}")
    sm, sn = vis.stride()
    if vis.numel() and not (((N == 1 or sn >= 1) and (M == 1 or sm >= N * sn)) or ((M == 1 or sm >= 1) and (N == 1 or sn >= M * sm))):
        raise ValueError(f"vis: strides {vis.stride()} of {tuple(vis.shape)} overlap")
    check(_props_occlude(_c(x), _c(normals), _c(directions), _c(targets), _c(clearance), ptr(bias), ptr(props), M, N, P, ptr(vis), max(sm, 0),
                         max(sn, 0), stream_ptr()), "nsky_props_occlude")


# ---- height fog and haze with shadowed sun shafts (relight/atmosphere.py, csrc/atmosphere.hip)
ATMOSPHERE_FLOATS = 12  # NSKY_ATMOSPHERE_FLOATS: density (0..2), albedo (3..5), H (0: homogeneous), base_height, g, far, background, -
ATMOSPHERE_MAX_SHAFTS = 64
_atmosphere_rows = _sig("nsky_atmosphere_rows", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                        C.c_void_p)
_atmosphere_apply = _sig("nsky_atmosphere_apply", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p)


def _atmosphere_block(params):
    assert params.shape == (ATMOSPHERE_FLOATS,) and params.dtype == torch.float32 and params.is_contiguous()


def atmosphere_rows(origins, directions, params, M: int, row_origins, row_directions, row_depth):
    """origins, directions: fp32 [R, 3]; params [12] (device) -> row_origins, row_directions [M R, 3], row_depth [M R]: row m R + r is ray r
    with the depth of the midpoint of segment m"""
    R = origins.shape[0]
    _atmosphere_block(params)
    assert 1 <= M <= ATMOSPHERE_MAX_SHAFTS and origins.shape == (R, 3) and directions.shape == (R, 3)
    assert row_origins.shape == (M * R, 3) and row_directions.shape == (M * R, 3) and row_depth.shape == (M * R,)
    assert all(x.dtype == torch.float32 for x in (origins, directions, row_origins, row_directions, row_depth))
    assert all(x.is_contiguous() for x in (row_origins, row_directions, row_depth))
    check(_atmosphere_rows(_c(origins), _c(directions), ptr(params), R, M, ptr(row_origins), ptr(row_directions), ptr(row_depth), stream_ptr()),
          "nsky_atmosphere_rows")


def atmosphere_apply(origins, directions, depth, accumulation, lin_in, background, abar, sun_dirs, sun_colours, vis, params, M: int, lin, rgb,
                     inscatter, transmittance, light_lin=None):
    """origins, directions: fp32 [R, 3]; depth, accumulation [R]; lin_in [Kb, R, 3] through its strides (the last one 1: a frame of K suns
    is ray-major in memory); background [R, 3] (one under all Kb) or [Kb, R, 3]; abar [Kb, 3]; sun_dirs, sun_colours [Kb, 3] or both None;
    vis [M, Kb, R] through its strides, or None; params [12] (device) -> lin, rgb, inscatter [Kb, R, 3] through the strides they share,
    transmittance [R, 3], and light_lin [R, 3] scaled in place, if given"""
    Kb, R, _ = lin_in.shape
    _atmosphere_block(params)
    assert 0 <= M <= ATMOSPHERE_MAX_SHAFTS and origins.shape == (R, 3) and directions.shape == (R, 3) and depth.numel() == R
    assert accumulation.numel() == R and background.shape in ((R, 3), (Kb, R, 3)) and abar.shape == (Kb, 3) and transmittance.shape == (R, 3)
    assert (sun_dirs is None) == (sun_colours is None) and (sun_dirs is None or (sun_dirs.shape == (Kb, 3) and sun_colours.shape == (Kb, 3)))
    assert vis is None or (sun_dirs is not None and M >= 1 and vis.shape == (M, Kb, R))
    assert light_lin is None or (light_lin.shape == (R, 3) and light_lin.is_contiguous())
    assert all(x is None or x.dtype == torch.float32 for x in (origins, directions, depth, accumulation, lin_in, background, abar, sun_dirs,
                                                                sun_colours, vis, lin, rgb, inscatter, transmittance, light_lin))
    ls_k, ls_r = _aa_strided(lin_in, Kb, R, 3, "the linear images")
    os_k, os_r = _aa_strided(lin, Kb, R, 3, "the fogged images")
    for x in (rgb, inscatter):
        if _aa_strided(x, Kb, R, 3, "the fogged images") != (os_k, os_r):
            raise ValueError(f"lin, rgb and inscatter share their strides, got {lin.stride()}, {rgb.stride()}, {inscatter.stride()}")
    vs = (0, 0, 0) if vis is None else vis.stride()
    assert transmittance.is_contiguous() and all(s >= 0 for s in vs)
    stride = 0 if background.dim() == 2 else R * 3
    check(_atmosphere_apply(_c(origins), _c(directions), _c(depth), _c(accumulation), ptr(lin_in), ls_k, ls_r, _c(background), stride, _c(abar),
                            _c(sun_dirs), _c(sun_colours), ptr(vis), vs[0], vs[1], vs[2], ptr(params), R, M, Kb, ptr(lin), ptr(rgb),
                            ptr(inscatter), os_k, os_r, ptr(transmittance), ptr(light_lin), stream_ptr()), "nsky_atmosphere_apply")


# ---- a display transform: metered exposure, bloom, tone curve, sRGB, 8 bits (relight/display.py, csrc/display.hip)
DISPLAY_BINS, DISPLAY_PARAMS, DISPLAY_MAX_RADIUS = 3072, 8, 96  # NSKY_DISPLAY_BINS / _PARAMS / _MAX_RADIUS
DISPLAY_CURVES = {"clamp": 0, "reinhard": 1, "aces": 2, "hable": 3}  # NSKY_DISPLAY_CLAMP ..
_display_histogram = _sig("nsky_display_histogram", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                          C.c_void_p)
_display_exposure = _sig("nsky_display_exposure", C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p)
_display_blur = _sig("nsky_display_blur", C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p)
_display_map = _sig("nsky_display_map", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                    C.c_void_p, C.c_void_p, C.c_void_p)


def _display_image(lin):
    if lin.dim() != 4 or lin.shape[3] != 3 or lin.dtype != torch.float32:
        raise ValueError(f"a linear image is float32 [K, H, W, 3], got {lin.dtype} {tuple(lin.shape)}")
    return lin.shape[0], lin.shape[1], lin.shape[2]


def _display_params(params):
    return ptr(_typed(params, torch.float32, DISPLAY_PARAMS))


def display_histogram(lin, mask, params, hist):
    """lin: fp32 [K, H, W, 3]; mask: fp32 [K, H, W] or None; params [8] (device) -> hist int64 [K, 3072], or [1, 3072] shared by the K
    images; the counts are added to what it holds"""
    K, H, W = _display_image(lin)
    rows = hist.shape[0] if hist.dim() == 2 else -1
    if rows not in (1, K) or hist.dtype != torch.int64 or hist.shape[1] != DISPLAY_BINS:
        raise ValueError(f"a histogram is int64 [{K}, {DISPLAY_BINS}] or [1, {DISPLAY_BINS}], got {hist.dtype} {tuple(hist.shape)}")
    check(_display_histogram(_c(lin), ptr(_typed(mask, torch.float32, K, H, W)), _display_params(params), H * W, K, int(rows == 1 and K > 1),
                             _c(hist), stream_ptr()), "nsky_display_histogram")


def display_exposure(hist, params, E):
    """hist: int64 [K, 3072]; params [8] -> E fp32 [K]"""
    K = hist.shape[0]
    check(_display_exposure(ptr(_typed(hist, torch.int64, K, DISPLAY_BINS)), _display_params(params), K, ptr(_typed(E, torch.float32, K)),
                            stream_ptr()), "nsky_display_exposure")


def _display_exposures(E, K):
    if E.dtype != torch.float32 or E.dim() != 1 or E.shape[0] not in (1, K) or not E.is_contiguous():
        raise ValueError(f"the exposures are float32 [{K}] or [1], got {E.dtype} {tuple(E.shape)}")
    return E.shape[0]


def display_blur(lin, E, params, weights, scratch, B):
    """lin: fp32 [K, H, W, 3]; E [K] or [1]; params [8]; weights fp32 [2 r + 1], 1 <= r <= 96 -> B [K, H, W, 3] through scratch (same shape)"""
    K, H, W = _display_image(lin)
    n = weights.numel()
    if weights.dim() != 1 or n % 2 != 1 or not 1 <= n // 2 <= DISPLAY_MAX_RADIUS:
        raise ValueError(f"2 r + 1 weights with r in 1..{DISPLAY_MAX_RADIUS}, got {tuple(weights.shape)}")
    check(_display_blur(_c(lin), ptr(E), _display_exposures(E, K), _display_params(params), ptr(_typed(weights, torch.float32, n)), n // 2, K, H,
                        W, ptr(_typed(scratch, torch.float32, K, H, W, 3)), ptr(_typed(B, torch.float32, K, H, W, 3)), stream_ptr()),
          "nsky_display_blur")


def display_map(lin, B, E, params, curve: str, rgb8, rgb=None):
    """lin: fp32 [K, H, W, 3]; B: the bloom (same shape) or None; E [K] or [1]; params [8]; curve: a key of DISPLAY_CURVES -> rgb8 uint8
    [K, H, W, 3] and, if given, rgb fp32 [K, H, W, 3]"""
    K, H, W = _display_image(lin)
    check(_display_map(_c(lin), ptr(_typed(B, torch.float32, K, H, W, 3)), ptr(E), _display_exposures(E, K), _display_params(params),
                       DISPLAY_CURVES[curve], H * W, K, ptr(_typed(rgb8, torch.uint8, K, H, W, 3)), ptr(_typed(rgb, torch.float32, K, H, W, 3)),
                       stream_ptr()), "nsky_display_map")


# ---- adaptive antialiasing of a frame: edge mask, sub-pixel rays, resolve (relight/antialias.py, csrc/antialias.hip)
_aa_edge_mask = _sig("nsky_aa_edge_mask", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                     C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p)
_aa_subpixel_rays = _sig("nsky_aa_subpixel_rays", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                         C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
_aa_resolve = _sig("nsky_aa_resolve", C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                   C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)


def aa_edge_mask(depth, normal, accumulation, lin, t_accumulation: float, t_depth: float, cos2: float, t_colour: float, covered: float, mask):
    """depth, accumulation: fp32 [H, W]; normal [H, W, 3]; lin: fp32 [K, H W, 3] through its strides (the last one 1), or None (no colour
    test); the thresholds of the rule by value (cos2 = cos^2 of the normals' angle) -> mask uint8 [H, W]"""
    if normal.dim() != 3 or normal.shape[2] != 3:
        raise ValueError(f"the normals of a frame are float32 [H, W, 3], got {tuple(normal.shape)}")
    H, W = normal.shape[0], normal.shape[1]
    K = 0 if lin is None else lin.shape[0]
    ls_k, ls_p = (0, 3) if lin is None else _aa_strided(lin, K, H * W, 3, "the linear images")
    check(_aa_edge_mask(ptr(_typed(depth, torch.float32, H, W)), ptr(_typed(normal, torch.float32, H, W, 3)),
                        ptr(_typed(accumulation, torch.float32, H, W)), ptr(lin), ls_k, ls_p, K, H, W, t_accumulation, t_depth, cos2, t_colour,
                        covered, ptr(_typed(mask, torch.uint8, H, W)), stream_ptr()), "nsky_aa_edge_mask")


def _aa_strided(t, K, P, Cn, what):
    """the strides (k, p) of fp32 [K, P, C] whose channels are contiguous and whose elements are all distinct addresses"""
    if t.dtype != torch.float32 or tuple(t.shape) != (K, P, Cn) or (Cn > 1 and t.stride(2) != 1):
        raise ValueError(f"{what} are float32 [{K}, {P}, {Cn}] with contiguous channels, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    sk, sp = t.stride(0), t.stride(1)
    k_major = (P == 1 or sp >= Cn) and (K == 1 or sk >= P * sp)
    p_major = (K == 1 or sk >= Cn) and (P == 1 or sp >= K * sk)
    if t.numel() and not (k_major or p_major):
        raise ValueError(f"{what}: strides {t.stride()} of {tuple(t.shape)} overlap")
    return sk, sp


def aa_subpixel_rays(origins, directions, norm, pixel_area, camera_indices, H: int, W: int, pixels, offsets, out_origins, out_directions,
                     out_norm, out_pixel_area=None, out_camera_indices=None):
    """a frame's flat bundle: origins, directions fp32 [H W, 3]; norm, pixel_area fp32 [H W, 1] or None; camera_indices int64 [H W, 1] or
    None; pixels int64 [E] (indices in [0, H W): the caller's to check); offsets fp32 [S1, 2] -> the same members for the E S1 rays"""
    P, E, S1 = H * W, pixels.shape[0], offsets.shape[0]
    N = E * S1
    check(_aa_subpixel_rays(ptr(_typed(origins, torch.float32, P, 3)), ptr(_typed(directions, torch.float32, P, 3)),
                            ptr(_typed(norm, torch.float32, P, 1)), ptr(_typed(pixel_area, torch.float32, P, 1)),
                            ptr(_typed(camera_indices, torch.int64, P, 1)), ptr(_typed(pixels, torch.int64, E)),
                            ptr(_typed(offsets, torch.float32, S1, 2)), H, W, E, S1, ptr(_typed(out_origins, torch.float32, N, 3)),
                            ptr(_typed(out_directions, torch.float32, N, 3)), ptr(_typed(out_norm, torch.float32, N, 1)),
                            ptr(_typed(out_pixel_area, torch.float32, N, 1)), ptr(_typed(out_camera_indices, torch.int64, N, 1)), stream_ptr()),
          "nsky_aa_subpixel_rays")


def aa_resolve(frame, samples, pixels, rgb=None):
    """frame: fp32 [K, P, C] through its strides (the last one 1: K may lead in the shape alone), in place; samples: fp32 [K, E, S1, C]
    through its strides (the last one 1); pixels: int64 [E], pairwise distinct; rgb: fp32 [K, P, C] through its strides, or None"""
    if frame.dim() != 3 or samples.dim() != 4:
        raise ValueError(f"a frame is [K, P, C] and its samples [K, E, S1, C], got {tuple(frame.shape)} and {tuple(samples.shape)}")
    K, P, Cn = frame.shape
    E, S1 = samples.shape[1], samples.shape[2]
    if samples.dtype != torch.float32 or tuple(samples.shape) != (K, E, S1, Cn) or (samples.numel() > 0 and Cn > 1 and samples.stride(3) != 1):
        raise ValueError(f"the samples are float32 [{K}, E, S1, {Cn}] with contiguous channels, got {samples.dtype} {tuple(samples.shape)} "
                         f"strides {samples.stride()}")
    xs_k, xs_e, xs_s = samples.stride(0), samples.stride(1), samples.stride(2)
    fs_k, fs_p = _aa_strided(frame, K, P, Cn, "a frame's values")
    rs_k, rs_p = (0, 0) if rgb is None else _aa_strided(rgb, K, P, Cn, "a frame's rgb")
    check(_aa_resolve(ptr(frame), fs_k, fs_p, ptr(samples), xs_k, xs_e, xs_s, ptr(_typed(pixels, torch.int64, E)), K, P, E, S1, Cn, ptr(rgb),
                      rs_k, rs_p, stream_ptr()), "nsky_aa_resolve")


# ---- depth of field of a frame: circle of confusion, mark, lens rays (relight/depth_of_field.py, csrc/dof.hip)
DOF_LENS_FLOATS = 12  # r^, s^, w^, a, 1 / z_f, a f_px
DOF_MAX_REACH = 64
_dof_coc = _sig("nsky_dof_coc", C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_void_p)
_dof_mark = _sig("nsky_dof_mark", C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p)
_dof_lens_rays = _sig("nsky_dof_lens_rays", C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                      C.c_void_p)


def dof_coc(depth, accumulation, lens, focus_pixel: int, covered: float, coc):
    """depth, accumulation: fp32 [H, W]; lens: fp32 [12] (with focus_pixel >= 0 its 1 / z_f is written from that pixel, on the device);
    focus_pixel: a flat index, or -1: lens[10] as it is -> coc fp32 [H, W]"""
    if depth.dim() != 2:
        raise ValueError(f"the depth of a frame is float32 [H, W], got {tuple(depth.shape)}")
    H, W = depth.shape
    if not -1 <= int(focus_pixel) < H * W:
        raise ValueError(f"focus_pixel: a flat index into {H} x {W} pixels or -1, got {focus_pixel}")
    check(_dof_coc(ptr(_typed(depth, torch.float32, H, W)), ptr(_typed(accumulation, torch.float32, H, W)),
                   ptr(_typed(lens, torch.float32, DOF_LENS_FLOATS)), H, W, int(focus_pixel), covered, ptr(_typed(coc, torch.float32, H, W)),
                   stream_ptr()), "nsky_dof_coc")


def dof_mark(coc, threshold: float, reach: int, mask):
    """coc: fp32 [H, W]; reach in 1..64 -> mask uint8 [H, W]"""
    if coc.dim() != 2:
        raise ValueError(f"the circles of confusion of a frame are float32 [H, W], got {tuple(coc.shape)}")
    H, W = coc.shape
    if not 1 <= int(reach) <= DOF_MAX_REACH:
        raise ValueError(f"reach is an integer in 1..{DOF_MAX_REACH}, got {reach!r}")
    check(_dof_mark(ptr(_typed(coc, torch.float32, H, W)), H, W, threshold, int(reach), ptr(_typed(mask, torch.uint8, H, W)), stream_ptr()),
          "nsky_dof_mark")


def dof_lens_rays(origins, directions, norm, pixel_area, camera_indices, H: int, W: int, pixels, table, lens, rotate: bool, out_origins,
                  out_directions, out_norm, out_pixel_area=None, out_camera_indices=None):
    """a frame's flat bundle as for aa_subpixel_rays; pixels int64 [E] (indices in [0, H W): the caller's to check); table fp32 [S1, 4] =
    (dx, dy, u, v); lens fp32 [12] -> the same members for the E S1 lens rays"""
    P, E, S1 = H * W, pixels.shape[0], table.shape[0]
    N = E * S1
    check(_dof_lens_rays(ptr(_typed(origins, torch.float32, P, 3)), ptr(_typed(directions, torch.float32, P, 3)),
                         ptr(_typed(norm, torch.float32, P, 1)), ptr(_typed(pixel_area, torch.float32, P, 1)),
                         ptr(_typed(camera_indices, torch.int64, P, 1)), ptr(_typed(pixels, torch.int64, E)),
                         ptr(_typed(table, torch.float32, S1, 4)), ptr(_typed(lens, torch.float32, DOF_LENS_FLOATS)), H, W, E, S1,
                         1 if rotate else 0, ptr(_typed(out_origins, torch.float32, N, 3)), ptr(_typed(out_directions, torch.float32, N, 3)),
                         ptr(_typed(out_norm, torch.float32, N, 1)), ptr(_typed(out_pixel_area, torch.float32, N, 1)),
                         ptr(_typed(out_camera_indices, torch.int64, N, 1)), stream_ptr()), "nsky_dof_lens_rays")
