"""Precomputed radiance transfer of one frame: bake the light-independent part of a camera's render once, relight it per light.

The renderer is linear in the light colours (csrc/transfer.hip, include/neusky_hip.h):
    T[r,d,c] = vis[r,d] sum_s w[r,s] alb[r,s,c] clamp(n[r,s].dir[d], 0, 1) / cnt[r,s]
    lin[r,c] = sum_d T[r,d,c] L[d,c] + bg[r,c] (1 - acc[r]);   rgb = clamp(linear_to_sRGB(lin), 0, 1)
`bake_transfer` runs the frame's chunked eval forward once and keeps T and acc; `RadianceTransfer.relight` then costs one streaming pass
over T per batch of up to 8 lights.  A new latent, environment map, rotation or exposure only changes L and bg.  A new camera needs a new
bake.  The identity needs the bake's light directions, so `fix_test_illumination_directions` must be on (the default)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import math

import torch

from .lighting import FrameLighting, light_colours, ray_background

STORAGES = ("fp32", "fp16")
LIGHTS_PER_PASS = 8
FRAME_KEYS = ("albedo", "accumulation", "depth", "p2p_dist", "normal")  # the light-independent outputs of the frame render
_BG_ROWS = 1 << 18  # rays per decoder pass of the latent background


def pack_fp16(T: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """scaled fp16 storage of T [R, ...]: (half(T[r] 2^e[r]), e int32 [R]) with e[r] chosen so that the row maximum of |T[r]| 2^e[r]
    lies in [0.5, 1); a row of zeros takes e = 0.  The scale is a power of two, so the only rounding is the one to fp16."""
    R = T.shape[0]
    mx = T.reshape(R, -1).abs().amax(dim=1) if T.numel() else T.new_zeros(R)
    _, x = torch.frexp(mx)  # mx = m 2^x, m in [0.5, 1)
    ok = (mx > 0) & torch.isfinite(mx)
    e = torch.where(ok, -x, torch.zeros_like(x)).to(torch.int32)
    scaled = torch.ldexp(T, e.reshape(R, *([1] * (T.dim() - 1))))
    return scaled.to(torch.float16), e


def unpack_fp16(half: torch.Tensor, exponents: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    R = half.shape[0]
    return torch.ldexp(half.to(dtype), -exponents.reshape(R, *([1] * (half.dim() - 1))))


def _storage_dtype(storage: str) -> torch.dtype:
    if storage not in STORAGES:
        raise ValueError(f"storage must be one of {STORAGES}, got {storage!r}")
    return torch.float32 if storage == "fp32" else torch.float16


def bake_rows(albedo, normals, weights, dirs, vis, storage: str) -> Dict[str, torch.Tensor]:
    """nsky_transfer_bake on one batch of rays (the inputs of the renderer: albedo, normals [R,S,3], weights [R,S], dirs [D,3],
    vis [R,D] or None) -> {"transfer": [R,D,3], "transfer_acc": [R,1], "transfer_exponents": int32 [R,1] (fp16 storage)}"""
    from .. import hip
    R, D = albedo.shape[0], dirs.shape[0]
    dev = albedo.device
    T = torch.empty(R, D, 3, dtype=_storage_dtype(storage), device=dev)
    acc = torch.empty(R, 1, dtype=torch.float32, device=dev)
    exps = torch.empty(R, 1, dtype=torch.int32, device=dev) if storage == "fp16" else None
    hip.transfer_bake(albedo.detach().contiguous(), normals.detach().contiguous(), weights.detach().contiguous(), dirs.contiguous(),
                      None if vis is None else vis.detach().contiguous(), T, 0, exps, acc)
    out = {"transfer": T, "transfer_acc": acc}
    if exps is not None:
        out["transfer_exponents"] = exps
    return out


def frame_light(model, envmap, dirs: torch.Tensor, ray_directions: torch.Tensor, cam: int,
                rotation: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(L [D, 3], bg [R, 3]) of one light of a baked frame: the frame render's own constructions (lighting.py), the latent background
    in blocks of _BG_ROWS rays"""
    L = light_colours(model, dirs, cam, rotation, envmap)
    if envmap is not None:
        from .envmap import envmap_lookup
        return L, envmap_lookup(envmap, ray_directions, rotation)
    R = ray_directions.shape[0]
    bg = torch.empty(R, 3, dtype=torch.float32, device=ray_directions.device)
    for a in range(0, R, _BG_ROWS):
        bg[a:a + _BG_ROWS] = ray_background(model, ray_directions[a:a + _BG_ROWS], cam, rotation)
    return L, bg


def relight_passes(baked, model, envmap, camera_index: Optional[int], rotations, exposure):
    """What `relight` of a baked frame (a RadianceTransfer or an SHRadianceTransfer) shares: (single, K, passes), `passes` yielding
    (k0, lights [kb, D, 3], bg [kb, R, 3]) for each pass of up to LIGHTS_PER_PASS lights."""
    if envmap is None and model is None:
        raise ValueError("relight needs an environment map, or a model whose illumination latent lights the frame")
    cam = baked.camera_index if camera_index is None else int(camera_index)
    single = rotations is None or (torch.is_tensor(rotations) and rotations.dim() == 2)
    rots = [rotations] if single else list(rotations)
    dev = baked.device
    rots = [None if r is None else torch.as_tensor(r, dtype=torch.float32).to(dev).reshape(3, 3) for r in rots]
    gain = None if exposure is None else torch.as_tensor(exposure, dtype=torch.float32).to(dev)
    R, D = baked.ray_directions.shape[0], baked.dirs.shape[0]
    K = len(rots)

    def passes():
        for k0 in range(0, K, LIGHTS_PER_PASS):
            kb = min(LIGHTS_PER_PASS, K - k0)
            lights = torch.empty(kb, D, 3, dtype=torch.float32, device=dev)
            bg = torch.empty(kb, R, 3, dtype=torch.float32, device=dev)
            for i in range(kb):
                L, b = frame_light(model, envmap, baked.dirs, baked.ray_directions, cam, rots[k0 + i])
                lights[i].copy_(L if gain is None else L * gain)
                bg[i].copy_(b if gain is None else b * gain)
            yield k0, lights, bg

    return single, K, passes()


class BakedFrame:
    """What the two baked frames share (RadianceTransfer below, transfer_sh.SHRadianceTransfer): the stored rows [R, n, 3] (fp32, or fp16
    with int32 row exponents [R]) under the attribute a subclass names, acc [R], the bake's light directions [D, 3], the rays' directions
    [R, 3] (for the background), the frame shape and the light-independent outputs of the frame render; the file of plain tensors; and the
    relight driver, whose per-pass kernel call is the subclass's `_relight_pass`."""
    ROWS = ""            # the stored rows: the attribute, the constructor argument and the key of a saved file
    FORMAT = 0           # "format" of a saved file
    EXTRA_KEYS = ()      # attributes of a subclass saved besides the shared ones: constructor arguments of the same names
    HAS_RESIDUAL = False  # whether _relight_pass returns the [kb] float64 residual of its lights (reported as "light_residual")

    def __init__(self, rows: torch.Tensor, exponents: Optional[torch.Tensor], acc: torch.Tensor, dirs: torch.Tensor,
                 ray_directions: torch.Tensor, shape: Sequence[int], outputs: Dict[str, torch.Tensor], camera_index: int,
                 fits: bool = True, others: str = ""):
        """fits: the subclass's own shape condition (rows against dirs); others: its own tensors' part of the shape message"""
        if rows.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"{self.ROWS} is stored as float32 or float16, not {rows.dtype}")
        if (rows.dtype == torch.float16) != (exponents is not None):
            raise ValueError("float16 storage comes with row exponents, float32 storage without")
        R, D = rows.shape[0], dirs.shape[0]
        if (not fits or rows.dim() != 3 or rows.shape[2] != 3 or tuple(dirs.shape) != (D, 3) or tuple(ray_directions.shape) != (R, 3)
                or acc.shape[0] != R):
            raise ValueError(f"{self.ROWS} {tuple(rows.shape)}, acc {tuple(acc.shape)}, {others}dirs {tuple(dirs.shape)}, "
                             f"rays {tuple(ray_directions.shape)}")
        if math.prod(int(v) for v in shape) != R:
            raise ValueError(f"frame shape {tuple(shape)} does not hold {R} rays")
        setattr(self, self.ROWS, rows)
        self.exponents, self.acc, self.dirs, self.ray_directions = exponents, acc.reshape(R), dirs, ray_directions
        self.shape = tuple(int(v) for v in shape)
        self.outputs = dict(outputs)
        self.camera_index = int(camera_index)

    @property
    def rows(self) -> torch.Tensor:
        return getattr(self, self.ROWS)

    @property
    def storage(self) -> str:
        return "fp32" if self.rows.dtype == torch.float32 else "fp16"

    @property
    def device(self) -> torch.device:
        return self.rows.device

    @property
    def nbytes(self) -> int:
        return self.rows.numel() * self.rows.element_size()

    # ------------------------------------------------------------------ persistence: plain tensors
    def save(self, path) -> None:
        state = {"format": self.FORMAT}
        for k in (self.ROWS, "exponents", "acc", *self.EXTRA_KEYS, "dirs", "ray_directions", "camera_index"):
            v = getattr(self, k)
            state[k] = v.cpu() if torch.is_tensor(v) else v
        state["shape"] = list(self.shape)
        state["outputs"] = {k: v.cpu() for k, v in self.outputs.items()}
        torch.save(state, path)

    @classmethod
    def load(cls, path, device: Union[str, torch.device] = "cuda"):
        state = torch.load(path, map_location="cpu", weights_only=True)
        if state.pop("format", None) != cls.FORMAT:
            raise ValueError(f"{path}: not a saved {cls.__name__}")
        state["outputs"] = {k: v.to(device) for k, v in state["outputs"].items()}
        return cls(**{k: v.to(device) if torch.is_tensor(v) else v for k, v in state.items()})

    # ------------------------------------------------------------------ relighting
    def _relight_pass(self, lights, bg, rgb, lin) -> Optional[torch.Tensor]:
        """the kernel call of one pass: lights [kb, D, 3] and bg [kb, R, 3] -> rgb and, unless None, lin [kb, R, 3]"""
        raise NotImplementedError

    @torch.no_grad()
    def relight(self, model=None, *, envmap=None, camera_index: Optional[int] = None, rotations=None, exposure=None,
                return_linear: bool = False, display=None) -> Dict[str, torch.Tensor]:
        """The frame under new light: the keys of get_outputs_for_camera_ray_bundle.  envmap: a relight.EnvironmentMap, else the
        illumination latent of `camera_index` (default: the bake's camera) of `model`.  rotations: None or one [3, 3] matrix -> rgb
        [*shape, 3]; a sequence or a [K, 3, 3] tensor -> rgb [K, *shape, 3], processed in batches of 8 lights per pass over the rows.
        exposure: a float or a 0-d tensor multiplying the light (on top of the map's own exposure).  display: a relight.DisplayTransform
        of the linear image, metered where acc exceeds its meter_mask_threshold: adds display_rgb8, display_rgb and display_exposure.
        A frame in a light basis adds "light_residual" ([K], or 0-d for a single light), a device tensor.  Nothing synchronises with
        the host."""
        from .display import frame_display
        single, K, passes = relight_passes(self, model, envmap, camera_index, rotations, exposure)
        R, dev = self.rows.shape[0], self.device
        rgb = torch.empty(K, R, 3, dtype=torch.float32, device=dev)
        lin = torch.empty(K, R, 3, dtype=torch.float32, device=dev) if return_linear or display is not None else None
        residual = torch.empty(K, dtype=torch.float64, device=dev) if self.HAS_RESIDUAL else None
        for k0, lights, bg in passes:
            kb = lights.shape[0]
            res = self._relight_pass(lights, bg, rgb[k0:k0 + kb], None if lin is None else lin[k0:k0 + kb])
            if residual is not None:
                residual[k0:k0 + kb] = res
        lead = () if single else (K,)
        out = {"rgb": rgb.view(*lead, *self.shape, 3)}
        if residual is not None:
            out["light_residual"] = residual[0] if single else residual
        if return_linear:
            out["linear"] = lin.view(*lead, *self.shape, 3)
        out.update(self.outputs)
        if display is not None:
            out.update(frame_display(display, lin.view(*lead, *self.shape, 3), self.shape, self.acc))
        return out


class RadianceTransfer(BakedFrame):
    """One baked frame: T [R, D, 3] (fp32, or fp16 with int32 row exponents [R]), acc [R], the bake's light directions [D, 3], the rays'
    directions [R, 3] (for the background), the frame shape, and the light-independent outputs of the frame render."""
    ROWS, FORMAT = "T", 1

    def __init__(self, T: torch.Tensor, exponents: Optional[torch.Tensor], acc: torch.Tensor, dirs: torch.Tensor,
                 ray_directions: torch.Tensor, shape: Sequence[int], outputs: Dict[str, torch.Tensor], camera_index: int = 0):
        super().__init__(T, exponents, acc, dirs, ray_directions, shape, outputs, camera_index, fits=T.shape[1:2] == dirs.shape[:1])

    def dense(self, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """T as a plain [R, D, 3] tensor (the fp16 rows unscaled)"""
        return self.T.to(dtype) if self.exponents is None else unpack_fp16(self.T, self.exponents, dtype)

    def _light(self, model, envmap, cam: int, rotation: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        """(L [D, 3], bg [R, 3]) of one light (frame_light)"""
        return frame_light(model, envmap, self.dirs, self.ray_directions, cam, rotation)

    def _relight_pass(self, lights, bg, rgb, lin) -> None:
        from .. import hip
        hip.transfer_relight(self.T, self.exponents, self.acc, lights, bg, rgb, lin)


def _bake_chunks(model, camera_ray_bundle, storage: str, chunk: Optional[int], use_graph: bool, camera_index: Optional[int], open_sink):
    """The chunk loop of a bake (bake_transfer, transfer_sh.bake_transfer_sh): the frame's chunked eval forward with the renderer's inputs
    routed into the transfer bake in `storage`.  open_sink(R, dirs, device) -> take(a, b, res), called after each chunk's forward with
    the chunk's result (res["transfer"], res["transfer_exponents"]: rows [a, b) of the frame in their first b - a rows).
    -> (shape, dirs, acc [R], ray directions [R, 3], outputs, camera_index)"""
    assert not model.training, "call model.eval() first"
    if not model.config.fix_test_illumination_directions:
        raise ValueError("bake_transfer needs fix_test_illumination_directions=True: a transfer is valid for the light directions it was "
                         "baked with, and with the option off every frame draws new ones")
    chunk = chunk or max(model.config.eval_num_rays_per_chunk, 4096)
    shape = tuple(camera_ray_bundle.origins.shape[:-1])
    flat = camera_ray_bundle.slice(0, 1 << 62)
    R = flat.origins.shape[0]
    if camera_index is None:
        camera_index = int(flat.camera_indices.reshape(-1)[0]) if flat.camera_indices is not None else 0
    dev = flat.origins.device
    runner = None
    try:
        model.frames.begin(camera_index, FrameLighting.of(bake=storage))
        dirs = model.frames.active.dirs.clone()
        take = open_sink(R, dirs, dev)
        acc = torch.empty(R, dtype=torch.float32, device=dev)
        outs = {k: [] for k in FRAME_KEYS}
        runner = model.frames.runner(chunk, flat, use_graph, cached=False)  # its own: a captured graph of this mode is never cached
        for a in range(0, R, chunk):
            b = min(a + chunk, R)
            res = runner.forward_rows(flat, a, b)
            take(a, b, res)
            acc[a:b].copy_(res["transfer_acc"][:b - a, 0])
            for k in FRAME_KEYS:
                outs[k].append(res[k][:b - a].clone())
    finally:
        model.frames.end()
        if runner is not None:
            runner.retire()
    outputs = {k: torch.cat(v).view(*shape, -1) for k, v in outs.items()}
    return shape, dirs, acc, flat.directions.reshape(R, 3).contiguous().clone(), outputs, camera_index


@torch.no_grad()
def bake_transfer(model, camera_ray_bundle, storage: str = "fp32", chunk: Optional[int] = None, use_graph: bool = True,
                  camera_index: Optional[int] = None) -> RadianceTransfer:
    """Run the chunked eval forward of get_outputs_for_camera_ray_bundle once, with the renderer's inputs routed into the transfer bake
    (the shading mode of this call's frame, models/frame.py: the plain frame render and its captured chunk graphs are untouched)."""
    dtype = _storage_dtype(storage)
    kept = {}

    def open_sink(R, dirs, dev):
        T = kept["T"] = torch.empty(R, dirs.shape[0], 3, dtype=dtype, device=dev)
        exps = kept["exps"] = torch.empty(R, dtype=torch.int32, device=dev) if storage == "fp16" else None

        def take(a, b, res):
            T[a:b].copy_(res["transfer"][:b - a])
            if exps is not None:
                exps[a:b].copy_(res["transfer_exponents"][:b - a, 0])
        return take

    shape, dirs, acc, rays, outputs, camera_index = _bake_chunks(model, camera_ray_bundle, storage, chunk, use_graph, camera_index, open_sink)
    return RadianceTransfer(kept["T"], kept["exps"], acc, dirs, rays, shape, outputs, camera_index)
