"""Illumination prior: direction sampler + RENI++-shaped decoder.

The reference imports both from the `reni` package (neusky/models/neusky_model.py:68-75), a git
submodule whose directory is EMPTY in the reference tree and whose pretrained weights are absent
 -> parity unpinned.  This module is this project's definition:
  * directions: D near-uniform unit vectors (Fibonacci lattice; reni uses an icosphere whose vertex count
    for `num_directions=512` is unknown) with an optional random SO(3) rotation (neusky_config.py:97-101);
  * decoder: FiLM-SIREN over a z-rotation-invariant representation of (latent Z [L,3], direction d):
    cond = per latent row (|Z_xy|, Z_z, Z_xy . d_xy), x = (|d_xy|, d_z) + NeRF(2 freqs); 3 log-HDR outputs;
    `unnormalise` = exp; per-image `scale` multiplies the HDR value.  Runs on ops.film_apply (MFMA).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Type

import numpy as np
import torch
from torch import nn

from ..fields.directional_distance_field import nerf_encoding
from ..utils.siren import FiLMSiren
from .. import ops
from ..plugin import ConfigBase


def fibonacci_sphere(n: int) -> torch.Tensor:
    i = torch.arange(n, dtype=torch.float64) + 0.5
    phi = torch.acos(1.0 - 2.0 * i / n)
    theta = math.pi * (1.0 + 5.0**0.5) * i
    d = torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], -1)
    return d.float()


def antipodal_sphere(n: int) -> torch.Tensor:
    """n (even) near-uniform unit directions that come in antipodal pairs {d, -d}, like the vertices of an
    icosphere (which is centrally symmetric).  Under ANY rotation exactly n/2 of them have z > 0, so the
    upper-hemisphere subset used for the DDF visibility (neusky_model.py:1650-1657) has a static size."""
    assert n % 2 == 0
    i = torch.arange(n // 2, dtype=torch.float64) + 0.5
    z = 1.0 - i / (n // 2)  # upper hemisphere, uniform in z
    r = torch.sqrt(1.0 - z * z)
    theta = math.pi * (1.0 + 5.0**0.5) * i
    up = torch.stack([r * torch.cos(theta), r * torch.sin(theta), z], -1)
    return torch.cat([up, -up], 0).float()


def icosphere_vertices(nu: int) -> torch.Tensor:
    """Vertices of the class-I geodesic icosahedron of subdivision frequency nu (10 nu^2 + 2 unit vectors, z up): what
    `icosphere.icosphere(nu)` returns to IcosahedronSampler (neusky/model_components/illumination_samplers.py:97; the
    `icosphere` package itself is absent here -> restated from its published construction, ordering parity unpinned):
    the 12 icosahedron vertices (0, +-1, +-phi) and cyclic shifts, every edge and face subdivided linearly into nu parts,
    all points pushed onto the unit sphere.  Order: base vertices, edge points, face-interior points.  The set is
    centrally symmetric, so under any rotation half of the off-equator vertices have z > 0."""
    assert nu >= 1
    phi = (1.0 + 5.0**0.5) / 2.0
    half = np.array([[0, 1, phi], [0, -1, phi], [1, phi, 0], [-1, phi, 0], [phi, 0, 1], [-phi, 0, 1]], dtype=np.float64)
    base = np.concatenate([half, -half], 0) / np.sqrt(1.0 + phi * phi)
    d2 = ((base[:, None] - base[None]) ** 2).sum(-1)
    edge2 = d2[d2 > 1e-9].min()
    adj = np.abs(d2 - edge2) < 1e-9
    edges = [(i, j) for i in range(12) for j in range(i + 1, 12) if adj[i, j]]
    faces = [(i, j, k) for i in range(12) for j in range(i + 1, 12) for k in range(j + 1, 12) if adj[i, j] and adj[j, k] and adj[i, k]]
    assert len(edges) == 30 and len(faces) == 20
    pts = [base]
    if nu > 1:
        w = np.arange(1, nu, dtype=np.float64)[:, None] / nu
        pts += [(1.0 - w) * base[i] + w * base[j] for i, j in edges]
        for i, j, k in faces:
            for a in range(1, nu - 1):
                for b in range(1, nu - a):
                    pts.append(((nu - a - b) * base[i] + a * base[j] + b * base[k])[None] / nu)
    v = np.concatenate(pts, 0)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    assert v.shape[0] == 10 * nu * nu + 2
    return torch.from_numpy(v).float()


_SKEW_BASIS: dict = {}


def random_rotation_device(device, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """uniform random SO(3) matrix from a unit quaternion (w, v), drawn and built on the device (no host round trip):
    R = (2 w^2 - 1) I + 2 (v v^T + w [v]x) in a dozen launches (the element-by-element form took 40)"""
    key = str(device)
    if key not in _SKEW_BASIS:
        k = torch.zeros(9, 3)
        for (i, j, c, sgn) in ((0, 1, 2, -1.0), (0, 2, 1, 1.0), (1, 0, 2, 1.0), (1, 2, 0, -1.0), (2, 0, 1, -1.0), (2, 1, 0, 1.0)):
            k[3 * i + j, c] = sgn  # [v]x = [[0,-z,y],[z,0,-x],[-y,x,0]]
        _SKEW_BASIS[key] = (k.to(device), torch.eye(3).to(device))
    K, eye = _SKEW_BASIS[key]
    q = torch.randn(4, device=device, generator=generator)
    q = q / q.norm()
    w, v = q[0], q[1:]
    return (2.0 * w * w - 1.0) * eye + 2.0 * (v[:, None] * v[None, :] + w * (K @ v).view(3, 3))


def random_rotation(generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """uniform random SO(3) matrix from a unit quaternion (host side, like the reference's scipy call)"""
    q = torch.randn(4, generator=generator, dtype=torch.float64)
    q = q / q.norm()
    w, x, y, z = q.tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float32)


@dataclass
class IcosahedronSamplerConfig(ConfigBase):
    _target: Type = field(default_factory=lambda: IcosahedronSampler)
    num_directions: int = 512
    apply_random_rotation: bool = True
    remove_lower_hemisphere: bool = False
    icosphere_order: Optional[int] = None
    """in-tree IcosahedronSamplerConfig member (illumination_samplers.py:77): when set, the direction set is the icosphere
    of that order (10 nu^2 + 2 vertices) and `num_directions` is ignored; None -> `num_directions` antipodal lattice points
    (reni's mapping from num_directions=512 to an order is not in the reference tree)"""

    def setup(self, **kwargs):
        return self._target(self, **kwargs)


class IcosahedronSampler:
    """returns directions [D,3] (host tensor; the model moves it to the device like neusky_model.py:456-458)"""

    def __init__(self, config: IcosahedronSamplerConfig):
        self.config = config
        self.icosphere_order = config.icosphere_order
        self._dev_cache = {}
        self._build()

    def _build(self) -> None:
        cfg = self.config
        d = icosphere_vertices(self.icosphere_order) if self.icosphere_order is not None else antipodal_sphere(cfg.num_directions)
        if cfg.remove_lower_hemisphere and not cfg.apply_random_rotation:
            d = d[d[:, 2] > 0]  # :117-118 (after the rotation there; a fixed set is filtered once)
        self.directions = d
        self._dev_cache = {}

    def set_icosphere_order(self, icosphere_order: int) -> None:
        """illumination_samplers.py:100-103"""
        self.icosphere_order = icosphere_order
        self._build()

    @staticmethod
    def icosphere_order_from_num_directions(num_directions: int) -> int:
        """illumination_samplers.py:105-107 (verbatim arithmetic: (n - 2) / 10 without the square root)"""
        return int((num_directions - 2) / 10)

    def on_device(self, device, apply_random_rotation: Optional[bool] = None, rotation: Optional[torch.Tensor] = None):
        """directions [D,3] on `device` (+ the indices of the D/2 with the largest z, ascending: for the antipodal set
        this IS the z > 0 subset).  Rotation drawn on the device; everything has static shapes (hipGraph-safe)."""
        key = str(device)
        if key not in self._dev_cache:
            self._dev_cache[key] = self.directions.to(device, torch.float32).contiguous()
        base = self._dev_cache[key]
        rot = self.config.apply_random_rotation if apply_random_rotation is None else apply_random_rotation
        D = base.shape[0]
        if (rotation is not None or rot) and not self.config.remove_lower_hemisphere and D % 2 == 0 and D <= 1024 \
                and (rotation is None or rotation.dim() == 2):
            # one kernel: rotation (drawn in the kernel, or the caller's), rotated set and its upper half (csrc/samplers.hip)
            from .. import hip
            from ..utils.utils import device_rng
            seed, counter = device_rng(self, "illumination_directions", 2, base.device)
            if getattr(self, "shared_across_ranks", False):  # camera-sharded decode: every rank draws the SAME rotation in a step
                from ..utils.utils import _rank
                seed = (int(seed) - 7919 * _rank()) & (2**63 - 1)
            dirs = torch.empty(D, 3, device=base.device)
            sel = torch.empty(D // 2, dtype=torch.int32, device=base.device)
            self.last_rotation = torch.empty(3, 3, device=base.device)
            hip.illumination_directions(base, None if rotation is None else rotation.to(base.device, torch.float32).contiguous(),
                                        seed, counter, dirs, sel, self.last_rotation)
            return dirs, sel
        if rotation is not None:
            rotation = rotation.to(device)
        elif rot:
            rotation = random_rotation_device(device)
        dirs = base if rotation is None else base @ rotation.T
        if self.config.remove_lower_hemisphere:
            if rotation is not None:
                raise NotImplementedError("remove_lower_hemisphere after a random rotation has a data-dependent size; use __call__")
            return dirs.contiguous(), torch.arange(dirs.shape[0], device=dirs.device, dtype=torch.int32)
        if rotation is None:
            # fixed (unrotated) set, e.g. eval with fix_test_illumination_directions: the reference's strict z > 0 mask
            # (neusky_model.py:1650-1657), computed once on the host -> static shape, equatorial vertices of an icosphere
            # (z == 0) stay in the lower set like there
            skey = key + ":sel"
            if skey not in self._dev_cache:
                self._dev_cache[skey] = torch.nonzero(self.directions[:, 2] > 0)[:, 0].to(torch.int32).to(device)
            return dirs.contiguous(), self._dev_cache[skey]
        # randomly rotated set: exactly D/2 directions have z > 0 for the centrally symmetric sets used here (ties on the
        # equator have probability zero), so the D/2 largest z ARE the z > 0 subset and the shape is static under a graph
        half = dirs.shape[0] // 2
        sel = torch.sort(torch.topk(dirs[:, 2], half).indices).values.to(torch.int32)
        return dirs.contiguous(), sel

    def __call__(self, apply_random_rotation: Optional[bool] = None, rotation: Optional[torch.Tensor] = None,
                 generator: Optional[torch.Generator] = None) -> torch.Tensor:
        rot = self.config.apply_random_rotation if apply_random_rotation is None else apply_random_rotation
        if rotation is None and rot:
            rotation = random_rotation(generator)
        d = self.directions if rotation is None else self.directions @ rotation.T.to(self.directions)
        if self.config.remove_lower_hemisphere and rotation is not None:
            d = d[d[:, 2] > 0]  # illumination_samplers.py:117-118
        return d


@dataclass
class RENIFieldConfig(ConfigBase):
    """subset of reni RENIFieldConfig used by neusky_config.py:78-96.  conditioning = "FiLM" (north star: 'RENI++ SIREN illumination
    decode'; what bench.py measures) or "Attention" (what neusky_config.py:79-80,90-91 selects: VN invariance, SO2 about z, transformer
    decoder with 8 heads x 6 layers, hidden 128)."""

    _target: Type = field(default_factory=lambda: RENIField)
    conditioning: str = "FiLM"
    invariant_function: str = "VN"
    equivariance: str = "SO2"
    axis_of_invariance: str = "z"
    latent_dim: int = 100
    hidden_features: int = 128
    hidden_layers: int = 9
    mapping_layers: int = 5
    mapping_features: int = 128
    num_attention_heads: int = 8
    num_attention_layers: int = 6
    fixed_decoder: bool = True
    trainable_scale: bool = True

    def setup(self, **kwargs):
        return self._target(self, **kwargs)


class AttentionDecoder(nn.Module):
    """RENI++ attention-conditioned decoder (neusky_config.py:78-95: conditioning="Attention", VN, SO2 about z, 8 heads x 6 layers,
    hidden 128).  The ns_reni source and its pretrained weights are absent from the reference tree: this is
    THIS PROJECT'S restatement of the published architecture -- direction-as-query cross-attention over the latent's invariant tokens --
    and stays PARITY UNPINNED (own float64 oracle: oracle.reni_attention_decode; SO(2)-equivariance property-tested).

      token n (one per latent row z_n):  t_n(d) = E [z_xy . d_xy,  z_x d_y - z_y d_x,  z_z,  |z_xy|] + e      (four z-rotation invariants of the pair)
      query:                             q_0(d) = X [|d_xy|, d_z, NeRF2(|d_xy|, d_z)] + x
      layer l:  q += Wo MHA(LN1(q); K = Wk t, V = Wv t)   (8 heads of 16, softmax(q k / 4));   q += W2 relu(W1 LN2(q))
      output:   log-HDR rgb = Wout LNf(q);   radiance = exp(.) * scale

    t_n is LINEAR in (d_x, d_y): t_n(d) = d_x A_n + d_y B_n + C_n with A, B, C functions of the latent only.  K and V of a camera are
    therefore three [L, H] matrices each (per layer), shared by all of its directions; the weights (d_x, d_y, 1) move to the query
    side, so scores and values for the D directions of a camera are dense products [D, 48] x [48, L] and [D, L] x [L, 48] per head
    -- the per-(camera, direction) token matrix (U D L H = 2 G floats per layer at 300 cameras x 512 directions) is never formed.  The batched products run on the matrix cores
    through the library GEMM (torch.bmm -> rocBLAS, exact fp32); this conditioning mode is outside the benchmarked step, which uses the
    FiLM-SIREN decoder on this package's own chain kernels."""

    def __init__(self, latent_dim: int, hidden: int = 128, heads: int = 8, layers: int = 6):
        super().__init__()
        assert hidden % heads == 0
        self.L, self.H, self.heads, self.n_layers = latent_dim, hidden, heads, layers
        self.token_embed = nn.Linear(4, hidden)
        self.query_embed = nn.Linear(10, hidden)
        self.layers = nn.ModuleList()
        for _ in range(layers):
            blk = nn.Module()
            blk.ln1, blk.ln2 = nn.LayerNorm(hidden), nn.LayerNorm(hidden)
            blk.wq, blk.wk, blk.wv, blk.wo = (nn.Linear(hidden, hidden) for _ in range(4))
            blk.ff1, blk.ff2 = nn.Linear(hidden, 2 * hidden), nn.Linear(2 * hidden, hidden)
            self.layers.append(blk)
        self.ln_f = nn.LayerNorm(hidden)
        self.out = nn.Linear(hidden, 3)

    def token_coefficients(self, latents: torch.Tensor):
        """latents [U, L, 3] -> A, B, C [U, L, H] with t_n(d) = d_x A_n + d_y B_n + C_n"""
        E, e = self.token_embed.weight, self.token_embed.bias  # [H, 4]
        zx, zy, zz = latents[..., 0:1], latents[..., 1:2], latents[..., 2:3]
        r = torch.sqrt(zx * zx + zy * zy + 1e-20)
        A = zx * E[:, 0] - zy * E[:, 1]
        B = zy * E[:, 0] + zx * E[:, 1]
        C = zz * E[:, 2] + r * E[:, 3] + e
        return A, B, C

    @staticmethod
    def _linear(x: torch.Tensor, lin: nn.Linear, act: str = "none") -> torch.Tensor:
        """lin(x) (+ ReLU) over the last dimension on this package's dense-layer kernels at any row count (fp32-grade fp16-split
        products, bias and activation in the epilogue; exact-fp32 input gradient); widths that are not multiples of 4 (the 10-wide query
        input, the 3-wide head) are zero padded"""
        K, N = lin.weight.shape[1], lin.weight.shape[0]
        rows = x.numel() // K
        Wp, bp = ops.pad_weight(lin.weight), ops.pad_bias(lin.bias)
        x2 = x.reshape(rows, K)
        if Wp.shape[1] != K:
            x2 = torch.nn.functional.pad(x2, (0, Wp.shape[1] - K))
        y = ops.DenseFn.apply(x2.contiguous(), Wp, bp, N, act, True)
        return y[:, :N].reshape(*x.shape[:-1], N)

    def _feed_forward(self, x: torch.Tensor, blk) -> torch.Tensor:
        frozen = not any(p.requires_grad for p in (blk.ff1.weight, blk.ff1.bias, blk.ff2.weight, blk.ff2.bias))
        if frozen and x.dim() == 2 and x.shape[1] % 4 == 0:
            return ops.FrozenFeedForwardFn.apply(x, blk.ff1.weight, blk.ff1.bias, blk.ff2.weight, blk.ff2.bias)
        return self._linear(self._linear(x, blk.ff1, "relu"), blk.ff2)

    def query_inputs(self, dirs: torch.Tensor) -> torch.Tensor:
        x = torch.stack([torch.sqrt(dirs[..., 0] ** 2 + dirs[..., 1] ** 2 + 1e-20), dirs[..., 2]], -1)
        return torch.cat([x, nerf_encoding(x, 2, 2.0)], -1)

    def forward(self, latents: torch.Tensor, dirs: torch.Tensor, ray_dirs: Optional[torch.Tensor] = None,
                ray_cam: Optional[torch.Tensor] = None):
        """latents [U, L, 3], dirs [U, D, 3] (the directions each latent is decoded at) -> log-HDR rgb [U, D, 3].
        With ray_dirs [R, 3] and ray_cam [R] (the latent each ray is decoded with): also the rays' rows, -> ([U, D, 3], [R, 3]).  A ray is
        one more direction of ITS camera: its row rides behind the U D grid rows through every row-local layer (layer norms, Wq, Wo, the
        feed-forward block) and attends to its camera's keys and values -- K~ / V~ are formed once per camera, not once per ray (decoding
        the rays as R one-direction cameras projects R x 3 L token rows per layer: twice the grid's own row count at 1024 rays)."""
        U, D = dirs.shape[:2]
        H, nh = self.H, self.heads
        dh = H // nh
        R = 0 if ray_dirs is None else ray_dirs.shape[0]
        N = U * D
        A, B, C = self.token_coefficients(latents)
        T3 = torch.cat([A, B, C], 1)  # [U, 3 L, H]
        all_dirs = dirs.reshape(N, 3) if R == 0 else torch.cat([dirs.reshape(N, 3), ray_dirs], 0)
        q = self.query_embed(self.query_inputs(all_dirs))  # [N + R, H]
        # t_n(d) = d_x A_n + d_y B_n + C_n makes every key / value a sum of three per-camera vectors weighted by (d_x, d_y, 1).  The
        # weights move to the QUERY side: q . k_n(d) = [d_x q | d_y q | q] . [kA_n | kB_n | kC_n], a contraction over 3 dh = 48 per head,
        # and sum_n p_n v_n(d) = d_x (p VA) + d_y (p VB) + (p VC): scores and values are ONE [D, 48] x [48, L] and ONE [D, L] x [L, 48]
        # product per head and camera; neither the [U, nh, D, 3, L] score parts nor a [D, 3 L] probability matrix is ever formed.
        L = self.L
        parts = lambda t: t.reshape(U, 3, L, nh, dh).permute(0, 3, 2, 1, 4).reshape(U, nh, L, 3 * dh)  # noqa: E731  [U, nh, L, (part, dh)]
        if dh != 16 or L > 128:
            raise NotImplementedError(f"attention core kernels (csrc/attention.hip): heads of 16 and at most 128 tokens, got {dh} / {L}")
        ray_cam = None if R == 0 else ray_cam.reshape(-1)
        ray_perm = ray_seg = None
        if R:  # the rays sorted by camera, for the per-camera ray kernels (device ops: graph-capturable)
            cam_sorted, ray_perm = torch.sort(ray_cam)
            ray_seg = torch.searchsorted(cam_sorted, torch.arange(U + 1, device=q.device)).to(torch.int32)
            ray_perm = ray_perm.to(torch.int32)

        resid = None  # the block's pending residual: added inside the next layer norm's pass (ops.add_layer_norm)
        mask = None
        for blk in self.layers:
            K3, V3 = self._linear(T3, blk.wk), self._linear(T3, blk.wv)  # [U, 3 L, H]
            # the bias of K / V belongs to the constant part only.  V: removed from the d_x and d_y thirds.  K: left where the linear
            # layer put it -- in the scores it adds (d_x + d_y) (q . b_k), the same number for every token of a row, and a softmax
            # does not see a per-row shift (nor does any gradient: the shift depends on no key) -- one [U, 3 L, H] pass less per layer
            if mask is None:
                mask = torch.cat([torch.ones(2 * L, device=T3.device), torch.zeros(L, device=T3.device)]).reshape(1, -1, 1)
            Kt, Vt = parts(K3), parts(V3 - blk.wv.bias * mask)
            q, n1 = ops.add_layer_norm(q, resid, blk.ln1)
            Qp = self._linear(n1, blk.wq)  # [N + R, H]
            # the attention core as HIP kernels (csrc/attention.hip: matrix-core forms from 32 directions per camera on, vector-unit forms
            # below): no [U, nh, D, L] score / probability matrices in memory
            O = ops.AttnCoreFn.apply(Qp, dirs, Kt, Vt, dh ** -0.5, ray_dirs, ray_perm, ray_seg)
            q, n2 = ops.add_layer_norm(q, self._linear(O, blk.wo), blk.ln2)
            resid = self._feed_forward(n2, blk)
        out = self.out(ops.add_layer_norm(q, resid, self.ln_f)[1])
        return out.reshape(U, D, 3) if R == 0 else (out[:N].reshape(U, D, 3), out[N:])


class RENIField(nn.Module):
    def __init__(self, config: RENIFieldConfig, num_train_data=None, num_eval_data=None, **_):
        super().__init__()
        if config.conditioning not in ("FiLM", "Attention"):
            raise NotImplementedError(f"RENI++ conditioning {config.conditioning!r}: FiLM or Attention")
        if config.conditioning == "Attention" and not (config.invariant_function == "VN" and config.equivariance == "SO2" and config.axis_of_invariance == "z"):
            raise NotImplementedError("the attention decoder is built for the configured VN / SO2-about-z invariance (neusky_config.py:79-91)")
        self.config = config
        self.latent_dim = config.latent_dim
        self.attention = config.conditioning == "Attention"
        if self.attention:
            self.network = AttentionDecoder(config.latent_dim, config.hidden_features, config.num_attention_heads, config.num_attention_layers)
            self.network.invalidate_weight_cache = lambda: None  # (no prepared-weight caches: model.begin_step calls it on every decoder)
        else:
            self.network = FiLMSiren(in_dim=2 + 8, hidden_layers=config.hidden_layers, hidden_features=config.hidden_features,
                                     mapping_network_in_dim=3 * config.latent_dim, mapping_network_layers=config.mapping_layers,
                                     mapping_network_features=config.mapping_features, out_dim=3)
        if config.fixed_decoder:
            for p in self.network.parameters():
                p.requires_grad_(False)

    @staticmethod
    def invariant_inputs(latents: torch.Tensor, dirs: torch.Tensor):
        zxy, zz = latents[..., :2], latents[..., 2]
        dxy, dz = dirs[..., :2], dirs[..., 2]
        cond = torch.stack([zxy.norm(dim=-1), zz, (zxy * dxy[:, None, :]).sum(-1)], -1).reshape(latents.shape[0], -1)
        x = torch.stack([dxy.norm(dim=-1), dz], -1)
        return cond, x

    def _decode(self, cond: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        x = torch.cat([x, nerf_encoding(x, 2, 2.0)], -1)
        x = torch.nn.functional.pad(x, (0, (-x.shape[1]) % 4)).contiguous()
        cond = torch.nn.functional.pad(cond, (0, (-cond.shape[1]) % 4)).contiguous()
        return torch.exp(self.network(x, cond, train_weights=not self.config.fixed_decoder))  # unnormalise (log-domain HDR)

    def forward_grid(self, directions: torch.Tensor, latent_codes: torch.Tensor, scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """every latent code against every direction: directions [D,3], latent_codes [U,L,3], scale [U] -> [U,D,3].
        Same arithmetic as forward() on the U*D pairs, built by broadcasting instead of gathering latents per pair."""
        U, L, _ = latent_codes.shape
        D = directions.shape[0]
        if self.attention:
            out = torch.exp(self.network(latent_codes, directions[None].expand(U, D, 3)))
            return out * scale[:, None, None] if scale is not None else out
        # both input matrices from one kernel (no [U D, 3 L] stack / pad copies)
        cond, x = ops.RENIGridInputsFn.apply(latent_codes, directions)
        out = torch.exp(self.network(x, cond, train_weights=not self.config.fixed_decoder)).reshape(U, D, 3)
        return out * scale[:, None, None] if scale is not None else out

    def forward_grid_and_rays(self, directions: torch.Tensor, latent_codes: torch.Tensor, scale: torch.Tensor,
                              ray_directions: torch.Tensor, ray_latent: torch.Tensor):
        """forward_grid(directions, latent_codes, scale) and forward(ray_directions, latent_codes[ray_latent], scale[ray_latent]) from
        ONE pass of the decoder: the rays' rows ride behind the U D grid rows (-> [U,D,3], [R,3])"""
        U, D = latent_codes.shape[0], directions.shape[0]
        if self.attention:  # the rays as extra directions of their cameras: one pass, keys / values once per camera
            grid, rays = self.network(latent_codes, directions[None].expand(U, D, 3), ray_directions, ray_latent)
            return torch.exp(grid) * scale[:, None, None], torch.exp(rays) * scale[ray_latent.reshape(-1)][:, None]
        cond, x = ops.RENIGridInputsFn.apply(latent_codes, directions, ray_directions, ray_latent)
        raw = self.network(x, cond, train_weights=not self.config.fixed_decoder, padded_output=True)
        return ops.RENIOutputFn.apply(raw, scale, ray_latent, U, D)  # exp + the per-image scale of both row sets

    def forward_camera(self, directions: torch.Tensor, latent: torch.Tensor, scale: Optional[torch.Tensor] = None,
                       rotation: Optional[torch.Tensor] = None) -> torch.Tensor:
        """B directions against ONE latent code: directions [B, 3], latent [L, 3], scale a scalar tensor -> [B, 3].  The same numbers as
        forward(directions, latent expanded to [B, L, 3], ...); the attention decoder forms the camera's keys / values once instead of
        once per direction (a render chunk is 4096 rays of one camera)."""
        if rotation is not None:
            directions = directions @ rotation.transpose(-1, -2)
        if self.attention:
            out = torch.exp(self.network(latent[None], directions[None])[0])
            return out * scale if scale is not None else out
        B = directions.shape[0]
        return self.forward(directions, latent[None].expand(B, -1, -1), None if scale is None else scale.expand(B))

    def forward(self, directions: torch.Tensor, latent_codes: torch.Tensor, scale: Optional[torch.Tensor] = None,
                rotation: Optional[torch.Tensor] = None) -> torch.Tensor:
        """directions [B,3], latent_codes [B,L,3], scale [B] -> HDR radiance [B,3] (already unnormalised)."""
        if rotation is not None:  # z-axis rotation of the illumination (render_animation.py:196-207)
            directions = directions @ (rotation if rotation.dim() == 2 else rotation).transpose(-1, -2)
        if self.attention:  # one direction per latent
            out = torch.exp(self.network(latent_codes, directions[:, None, :])[:, 0])
            return out * scale[:, None] if scale is not None else out
        cond, x = self.invariant_inputs(latent_codes, directions)
        out = self._decode(cond, x)
        return out * scale[:, None] if scale is not None else out
