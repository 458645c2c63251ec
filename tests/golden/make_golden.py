"""Generate the golden vectors under tests/golden/*.npz by IMPORTING the reference's in-tree
functions (read-only mount at /root/reference) in the build container.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py

Only data (seeded inputs are rebuilt by tests/golden/inputs.py; outputs are stored) is committed;
the reference itself never travels.  Each block names the reference symbol it calls (file:line).
External dependencies of the reference that are absent here (nerfstudio, reni, tcnn) are replaced
by explicit analytic STAND-INS defined below, so these vectors pin the reference's in-tree
arithmetic and index plumbing and nothing else.
"""
from __future__ import annotations

import functools
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stub_importer  # noqa: E402
import inputs as gi  # noqa: E402

_ref_stub_importer.install()

import neusky.utils.utils as ru  # noqa: E402
import neusky.utils.siren as rsiren  # noqa: E402
import neusky.model_components.renderers as rr  # noqa: E402
import neusky.model_components.losses as rl  # noqa: E402
import neusky.model_components.ddf_sampler as rsamp  # noqa: E402
import neusky.fields.sdf_albedo_field as rsdf  # noqa: E402
import neusky.fields.directional_distance_field as rddf  # noqa: E402
import neusky.models.ddf_model as rdm  # noqa: E402
import neusky.models.neusky_model as rnm  # noqa: E402

T = torch.from_numpy
NS = types.SimpleNamespace


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  ({os.path.getsize(path)/1024:.1f} KiB)")


class Bag:
    """attribute bag standing in for nerfstudio RayBundle / RaySamples / Frustums."""

    def __init__(self, **k):
        self.__dict__.update(k)

    def to(self, *_a, **_k):
        return self


# ----------------------------------------------------------------------------- G1
def g1_srgb():
    # neusky/utils/utils.py:11-31
    x = np.concatenate([
        np.array([-1.0, -1e-3, 0.0, 1e-8, 0.0031308 - 1e-7, 0.0031308, 0.0031308 + 1e-7, 0.5, 1.0, 1.5, 40.0]),
        np.linspace(0.0, 1.2, 53),
    ]).astype(np.float32)
    y = ru.linear_to_sRGB(T(x))
    save("g1_srgb", x=x, y=y)


# ----------------------------------------------------------------------------- G2
def g2_sphere():
    g = gi.rng(2)
    p = g.uniform(-0.6, 0.6, (64, 3)).astype(np.float32)
    d_unit = gi.unit(g.normal(size=(64, 3))).astype(np.float32)
    d_raw = (d_unit * g.uniform(0.3, 3.0, (64, 1))).astype(np.float32)
    # grazing / outside cases for the clamped variant
    p2 = p.copy()
    p2[:4] = np.array([[1.2, 0, 0], [0, 1.0, 0], [0.999, 0, 0.04], [0, 0, -1.5]], np.float32)
    # torch's float32 sqrt on the CPU is not correctly rounded and its last bit depends on the CPU model: every (argument, result)
    # of the reference's torch.sqrt calls is kept in g2_sqrt, so a test on another CPU can replay the generating CPU's roundings
    calls, sqrt = [], torch.sqrt

    def recording_sqrt(x):
        y = sqrt(x)
        calls.append((x.numpy().ravel().copy(), y.numpy().ravel().copy()))
        return y

    torch.sqrt = recording_sqrt
    try:
        # free function neusky/utils/utils.py:68-93 (no normalisation, no clamp) -> inside-sphere unit dirs only
        y_free = ru.ray_sphere_intersection(T(p), T(d_unit), 1.0)
        # method neusky/models/neusky_model.py:1590-1622 (normalises, clamps discriminant)
        y_meth = rnm.NeuSkyFactoModel.ray_sphere_intersection(None, T(p2), T(d_raw), 1.0)
        y_meth_r2 = rnm.NeuSkyFactoModel.ray_sphere_intersection(None, T(p2), T(d_raw), 2.0)
    finally:
        torch.sqrt = sqrt
    save("g2_sphere", p=p, d_unit=d_unit, d_raw=d_raw, p2=p2, y_free=y_free, y_meth=y_meth, y_meth_r2=y_meth_r2)
    save("g2_sqrt", x=np.concatenate([c[0] for c in calls]), y=np.concatenate([c[1] for c in calls]))


# ----------------------------------------------------------------------------- G3
def _lambertian_ref(inp, training=True):
    R, S, _ = inp["albedo"].shape
    D = inp["dirs"].shape[0]
    N = R * S
    # broadcast exactly as the reference materialises them (neusky_model.py:512-525, 1755-1759)
    light_dirs = T(inp["dirs"])[None].expand(N, D, 3).contiguous()
    cols = T(inp["cam_colours"])[T(inp["cam_of_ray"])]  # [R,D,3]
    light_cols = cols[:, None].expand(R, S, D, 3).reshape(N, D, 3).contiguous()
    vis = T(inp["vis"])[:, None, :, None].expand(R, S, D, 1).reshape(N, D, 1).contiguous()
    mod = rr.RGBLambertianRendererWithVisibility()
    mod.train(training)
    # neusky/model_components/renderers.py:60-130 (+ eval clamp :173-174)
    return mod(
        albedos=T(inp["albedo"]).clone(), normals=T(inp["normals"]).clone(), light_directions=light_dirs,
        light_colors=light_cols, visibility=vis, background_illumination=T(inp["bg"]),
        weights=T(inp["weights"])[..., None],
    )


def g3_lambertian():
    small = gi.lambertian_inputs(seed=3, R=8, S=4, D=16, U=3)
    save("g3_lambertian_small", rgb_train=_lambertian_ref(small, True), rgb_eval=_lambertian_ref(small, False),
         **small)
    big = gi.lambertian_inputs(seed=33, R=64, S=96, D=512, U=11)
    chk = float(sum(np.asarray(v, np.float64).sum() for v in big.values()))
    save("g3_lambertian_big", rgb_train=_lambertian_ref(big, True), input_checksum=np.float64(chk),
         shape=np.array([64, 96, 512, 11]), seed=np.array(33))


# ----------------------------------------------------------------------------- G4
def standin_ddf(origins: torch.Tensor, directions: torch.Tensor, radius: float):
    """Analytic stand-in for the DDF: distance from the sphere point along the ray to the plane
    z = 0.1 (clamped to [0, 2r]); sdf stand-in = z of the termination point minus 0.1."""
    oz, dz = origins[:, 2], directions[:, 2]
    t = torch.where(dz < -1e-6, (0.1 - oz) / dz.clamp(max=-1e-6), torch.full_like(oz, 2 * radius))
    t = t.clamp(0.0, 2 * radius)
    sdf = (origins + directions * t[:, None])[:, 2:3] - 0.1
    return t, sdf


def g4_visibility():
    for tag, (only_upper, lower_vis, shadow) in {
        "upper_lower1": (True, True, False), "upper_lower0": (True, False, False), "all_shadow": (False, True, True),
    }.items():
        inp = gi.visibility_inputs(seed=4, R=16, S=3, D=42, n_outside=2)
        radius = 1.0
        R, S, D = 16, 3, 42
        rnm.RayBundle = Bag  # neusky_model.py:1705-1709 constructs RayBundle(origins=, directions=, pixel_area=)

        def vis_field(rb, batch=None, neusky=None, stop_gradients=True):
            t, sdf = standin_ddf(rb.origins, rb.directions, radius)
            return {"expected_termination_dist": t, "sdf_at_termination": sdf}

        self = NS(
            config=NS(only_upperhemisphere_visibility=only_upper, lower_hermisphere_visibility=lower_vis,
                      sdf_to_visibility_stop_gradients="depth"),
            ddf_radius=radius, visibility_field=vis_field,
        )
        self.ray_sphere_intersection = functools.partial(rnm.NeuSkyFactoModel.ray_sphere_intersection, self)
        ray_samples = Bag(frustums=Bag(origins=T(inp["origins"]).clone(), directions=T(inp["directions"]).clone()))
        illum = T(inp["dirs"])[None].expand(R * S, D, 3).contiguous()
        # neusky/models/neusky_model.py:1624-1778
        out = rnm.NeuSkyFactoModel.compute_visibility(
            self, ray_samples=ray_samples, depth=T(inp["depth"]).clone(), illumination_directions=illum,
            threshold_distance=torch.tensor(0.35), sigmoid_scale=torch.tensor(25.0), compute_shadow_map=shadow,
        )
        extra = {"difference": out["difference"]} if shadow else {}
        save(f"g4_visibility_{tag}", visibility=out["visibility"],
             expected_termination_dist=out["expected_termination_dist"],
             termination_dist=out["visibility_batch"]["termination_dist"],
             sdf_at_termination=out["visibility_batch"]["sdf_at_termination"],
             threshold=np.float32(0.35), scale=np.float32(25.0), **extra)


# ----------------------------------------------------------------------------- G5
def g5_local_frame():
    inp = gi.sphere_rays(seed=5, M=48, radius=1.0)
    p, d = T(inp["positions"]), T(inp["directions"])
    # neusky/models/ddf_model.py:158-181 and the einsum at :200
    rot = rdm.DDFModel.get_localised_transforms(None, p)
    d_loc = torch.einsum("ijl,ij->il", rot, d)
    save("g5_local_frame", rot=rot, d_loc=d_loc)


# ----------------------------------------------------------------------------- G6 / DDF model plumbing
def nerf_encoding_standin(x: torch.Tensor, num_freq: int, max_exp: float, include_input: bool):
    """OUR restatement of nerfstudio NeRFEncoding - stand-in, not reference code."""
    freqs = 2.0 ** torch.linspace(0.0, max_exp, num_freq, dtype=x.dtype)
    xs = 2.0 * torch.pi * x[..., None] * freqs
    xs = xs.reshape(*x.shape[:-1], -1)
    enc = torch.sin(torch.cat([xs, xs + torch.pi / 2.0], -1))
    return torch.cat([x, enc], -1) if include_input else enc


def g6_ddf_field_and_model():
    inp = gi.sphere_rays(seed=6, M=40, radius=1.0)
    p, d = T(inp["positions"]), T(inp["directions"])
    g = gi.rng(66)
    Wp = T(g.normal(size=(3, 32)).astype(np.float32))

    def pos_enc(x):  # stand-in for tcnn hash encoding (absent): smooth 32-d feature of position
        return torch.sin(x @ Wp)

    Wd = T(g.normal(size=(15, 1)).astype(np.float32) * 0.3)
    Wc = T(g.normal(size=(35, 1)).astype(np.float32) * 0.3)

    def ddf_net(x, conditioning_input):  # stand-in for reni FiLMSiren (absent)
        return x @ Wd + torch.tanh(conditioning_input @ Wc)

    field_self = NS(
        position_encoding=pos_enc,
        direction_encoding=lambda x: nerf_encoding_standin(x, 2, 2.0, False),
        ddf=ddf_net, ddf_radius=1.0, termination_output_activation=torch.sigmoid,
        config=NS(conditioning="FiLM", ddf_type="ddf", predict_probability_of_hit=False),
    )
    field_self.forward = functools.partial(rddf.DirectionalDistanceField.get_outputs, field_self)

    rdm.RaySamples = Bag
    rdm.Frustums = Bag
    gm = gi.rng(67)
    mv_points = gi.unit(gm.normal(size=(40, 3))).astype(np.float32)
    rdm.random_points_on_unit_sphere = lambda num_points: T(mv_points).clone()
    sky = gi.visibility_inputs(seed=68, R=12, S=1, D=4, n_outside=0)
    sky_o, sky_d = sky["origins"][:, 0], sky["directions"][:, 0]
    term = gm.uniform(0.2, 1.5, (40, 1)).astype(np.float32)
    mask = (gm.uniform(size=(40, 1)) > 0.3).astype(np.float32)

    def sdf_standin(x):
        return (x.norm(dim=-1, keepdim=True) - 0.5)

    model_self = NS(
        field=field_self, training=True, ddf_radius=1.0,
        config=NS(compute_normals=False, include_depth_loss_scene_center_weight=True,
                  scene_center_weight_include_z=False, scene_center_weight_exp=3.0,
                  loss_inclusions={"depth_l1_loss": True, "depth_l2_loss": False, "sdf_l1_loss": False,
                                   "sdf_l2_loss": True, "prob_hit_loss": False, "normal_loss": False,
                                   "multi_view_loss": True, "sky_ray_loss": True},
                  mask_to_circumference=False, inverse_depth_weight=False,
                  loss_coefficients={}),
        depth_l1_loss=torch.nn.L1Loss(reduction="none"), sdf_l2_loss=torch.nn.MSELoss(),
        multi_view_loss=torch.nn.MSELoss(), sky_ray_loss=torch.nn.L1Loss(),
    )
    model_self.get_localised_transforms = functools.partial(rdm.DDFModel.get_localised_transforms, model_self)
    batch = {"termination_dist": T(term), "mask": T(mask),
             "sky_ray_bundle": Bag(origins=T(sky_o), directions=T(sky_d))}
    neusky = NS(field=NS(get_sdf_at_pos=sdf_standin))
    # neusky/models/ddf_model.py:183-369 (field call -> directional_distance_field.py:261-306)
    out = rdm.DDFModel.get_outputs(model_self, Bag(origins=p, directions=d), batch, neusky, stop_gradients=False)
    rdm.misc = NS(scale_dict=lambda dct, coeff: dct)  # scaling restated + tested separately
    # neusky/models/ddf_model.py:407-493
    losses = rdm.DDFModel.get_loss_dict(model_self, out, batch)
    save("g6_ddf", Wp=Wp, Wd=Wd, Wc=Wc, mv_points=mv_points, sky_o=sky_o, sky_d=sky_d, term=term, mask=mask,
         **{f"out_{k}": v for k, v in out.items()}, **{f"loss_{k}": v for k, v in losses.items()})


# ----------------------------------------------------------------------------- G7 losses
def monosdf_normal_loss_standin(normal_pred, normal_gt):
    """OUR restatement of nerfstudio monosdf_normal_loss (external) - stand-in."""
    normal_gt = torch.nn.functional.normalize(normal_gt, p=2, dim=-1)
    normal_pred = torch.nn.functional.normalize(normal_pred, p=2, dim=-1)
    l1 = torch.abs(normal_pred - normal_gt).sum(dim=-1).mean()
    cos = (1.0 - torch.sum(normal_pred * normal_gt, dim=-1)).mean()
    return l1 + cos


def g7_losses():
    g = gi.rng(7)
    R, S = 32, 6
    rgb = g.uniform(0, 1, (R, 3)).astype(np.float32)
    image = g.uniform(0, 1, (R, 3)).astype(np.float32)
    mask = np.stack([g.uniform(size=R) < 0.9, g.uniform(size=R) < 0.6, g.uniform(size=R) < 0.15,
                     g.uniform(size=R) < 0.3], -1)
    mask[:, 1] &= ~mask[:, 3]
    eik = g.normal(0, 1, (R, S, 3)).astype(np.float32)
    w = g.uniform(0, 0.3, (R, S, 1)).astype(np.float32)
    w[0] = 0.0
    w[1] = 0.5  # sum > 1 -> clip
    normal = g.normal(0, 1, (R, 3)).astype(np.float32)
    hdr_bg = np.exp(g.normal(0, 1, (R, 3))).astype(np.float32)
    grid_density = g.uniform(0, 1, (50, 1)).astype(np.float32)
    sdf_term = g.normal(0, 0.2, (R * 4, 1)).astype(np.float32)

    # neusky/model_components/losses.py:44-58
    sky = rl.RENISkyPixelLoss(alpha=0.1)
    m3 = T(mask[:, 3].astype(np.float32))[:, None].expand(R, 3)
    sky_val = sky(inputs=ru.linear_to_sRGB(T(hdr_bg)), targets=T(image), mask=m3)

    rnm.monosdf_normal_loss = monosdf_normal_loss_standin
    rnm.misc = NS(scale_dict=lambda dct, coeff: dct)
    rnm.linear_to_sRGB = ru.linear_to_sRGB  # reni copy absent; in-tree copy has identical text (utils.py:11-31)
    incl = {
        "rgb_l1_loss": True, "rgb_l2_loss": False, "cosine_colour_loss": False, "eikonal loss": True,
        "fg_mask_loss": True, "normal_loss": False, "depth_loss": False, "sdf_level_set_visibility_loss": True,
        "interlevel_loss": False,  # external nerfstudio fn: restated + property-tested separately
        "sky_pixel_loss": {"enabled": True, "cosine_weight": 0.1},
        "hashgrid_density_loss": {"enabled": True, "grid_resolution": 10}, "ground_plane_loss": True,
        "visibility_sigmoid_loss": {"visibility_threshold_method": "learnable", "optimise_sigmoid_bias": True,
                                    "optimise_sigmoid_scale": False, "target_min_bias": 0.1,
                                    "target_max_scale": 25, "steps_until_min_bias": 50000},
    }
    self = NS(
        device="cpu", training=True, fitting_eval_latents=False,
        config=NS(loss_inclusions=incl, loss_coefficients={}),
        rgb_l1_loss=torch.nn.L1Loss(), sky_pixel_loss=sky, hashgrid_density_loss=torch.nn.L1Loss(),
        ground_plane_loss=monosdf_normal_loss_standin, visibility_sigmoid_loss=torch.nn.MSELoss(),
        sdf_level_set_visibility_loss=torch.nn.MSELoss(), visibility_threshold_method="learnable",
        visibility_threshold=torch.tensor(2.0), sigmoid_scale=torch.tensor(25.0),
    )
    outputs = {"rgb": T(rgb), "eik_grad": T(eik), "weights": T(w), "normal": T(normal),
               "hdr_background_colours": T(hdr_bg), "grid_density": T(grid_density),
               "sdf_at_termination": T(sdf_term)}
    batch = {"image": T(image), "mask": T(mask)}
    # neusky/models/neusky_model.py:933-1035 (train branch)
    ld = rnm.NeuSkyFactoModel.get_loss_dict(self, outputs, batch)
    # neusky/models/neusky_model.py:1036-1059 (the other branch: evaluation / eval-latent fitting, per-image latents)
    self.fitting_eval_latents = True
    self.config.eval_latent_optimise_method = "per_image"
    self.rgb_l2_loss = torch.nn.MSELoss()
    self.cosine_colour_loss = torch.nn.CosineSimilarity(dim=1)
    ld_eval = rnm.NeuSkyFactoModel.get_loss_dict(self, outputs, batch)
    incl2 = dict(incl, rgb_l2_loss=True, cosine_colour_loss=True)  # every term the branch can emit
    self.config.loss_inclusions = incl2
    ld_eval_all = rnm.NeuSkyFactoModel.get_loss_dict(self, outputs, batch)
    self.config.eval_latent_optimise_method = "nerf_osr_envmap"  # :1048: no sky-pixel term
    ld_eval_osr = rnm.NeuSkyFactoModel.get_loss_dict(self, outputs, batch)
    save("g7_losses", rgb=rgb, image=image, mask=mask, eik=eik, w=w, normal=normal, hdr_bg=hdr_bg,
         grid_density=grid_density, sdf_term=sdf_term, sky_direct=sky_val,
         **{f"loss_{k}": v for k, v in ld.items()}, **{f"evalloss_{k}": v for k, v in ld_eval.items()},
         **{f"evalall_{k}": v for k, v in ld_eval_all.items()}, **{f"evalosr_{k}": v for k, v in ld_eval_osr.items()})


# ----------------------------------------------------------------------------- G8 FiLM-SIREN
from make_golden_weights import film_siren_weights  # noqa: E402


def g8_film_siren():
    for tag, (hidden, layers, mh, ml, M) in {"small": (32, 3, 32, 2, 24), "full": (256, 5, 256, 5, 64)}.items():
        in_dim, map_in = 15, 35
        # neusky/utils/siren.py:147-208
        net = rsiren.DDFFiLMSiren(input_dim=in_dim, mapping_network_input_dim=map_in, siren_hidden_features=hidden,
                                  siren_hidden_layers=layers, mapping_network_features=mh,
                                  mapping_network_layers=ml, out_features=1)
        w = film_siren_weights(80 + hidden, in_dim, map_in, hidden, layers, mh, ml, 1)
        with torch.no_grad():
            lin = [m for m in net.mapping_network.network if isinstance(m, torch.nn.Linear)]
            for i in range(ml):
                lin[i].weight.copy_(T(w[f"map_w{i}"])); lin[i].bias.copy_(T(w[f"map_b{i}"]))
            lin[-1].weight.copy_(T(w["map_wo"])); lin[-1].bias.copy_(T(w["map_bo"]))
            for i in range(layers):
                net.net[i].layer.weight.copy_(T(w[f"film_w{i}"])); net.net[i].layer.bias.copy_(T(w[f"film_b{i}"]))
            net.final_layer.weight.copy_(T(w["out_w"])); net.final_layer.bias.copy_(T(w["out_b"]))
        g = gi.rng(81)
        cond = g.uniform(-1, 1, (M, map_in)).astype(np.float32)
        x = g.uniform(-1, 1, (M, in_dim)).astype(np.float32)
        with torch.no_grad():
            y = net(torch.cat([T(cond), T(x)], -1))
            freq, phase = net.mapping_network(T(cond))
        save(f"g8_film_siren_{tag}", cond=cond, x=x, y=y, freq_raw=freq[:, :8], phase=phase[:, :8],
             cfg=np.array([in_dim, map_in, hidden, layers, mh, ml, 1, 80 + hidden]))


# ----------------------------------------------------------------------------- G9 illumination plumbing
def g9_sample_illumination():
    g = gi.rng(9)
    R, S, D, NT, L = 12, 3, 10, 7, 5
    cam = g.integers(0, NT, (R,)).astype(np.int64)
    cam_rs = np.repeat(cam[:, None, None], S, 1)  # [R,S,1]
    ray_dirs = gi.unit(g.normal(size=(R, 3))).astype(np.float32)
    latents = g.normal(0, 0.5, (NT, L, 3)).astype(np.float32)
    scales = g.uniform(0.5, 2.0, (NT,)).astype(np.float32)
    dirs = gi.fibonacci_sphere(D)
    A = g.normal(0, 1, (L, 3)).astype(np.float32)

    class RaySamplesBag(Bag):
        def __getitem__(self, idx):
            return RaySamplesBag(frustums=Bag(directions=self.frustums.directions[idx]),
                                 camera_indices=self.camera_indices[idx])

        @property
        def shape(self):
            return self.frustums.directions.shape[:-1]

    class StandInRENI(rnm.RENIField):  # passes isinstance(self.illumination_field, RENIField) :482
        def __init__(self):
            pass

        def forward(self, ray_samples, latent_codes, scale, rotation=None):
            d = ray_samples.frustums.directions
            proj = torch.einsum("blc,bc->bl", latent_codes, d)  # [B,L]
            rgb = torch.tanh(proj @ T(A)) * scale[:, None]
            return {rnm.RENIFieldHeadNames.RGB: rgb}

        def unnormalise(self, x):
            return torch.exp(x)

    self = NS(
        training=True, device="cpu", config=NS(fix_test_illumination_directions=True),
        illumination_field=StandInRENI(),
        illumination_sampler=lambda **k: RaySamplesBag(frustums=Bag(directions=T(dirs).clone()),
                                                        camera_indices=None),
        get_illumination_field=lambda: (T(latents), T(scales)),
    )
    ray_samples = RaySamplesBag(
        frustums=Bag(directions=T(ray_dirs)[:, None, :].expand(R, S, 3).contiguous()),
        camera_indices=T(cam_rs),
    )
    # neusky/models/neusky_model.py:445-551
    cols, idirs, bg = rnm.NeuSkyFactoModel.sample_illumination(self, ray_samples, None)
    save("g9_sample_illumination", cam=cam, ray_dirs=ray_dirs, latents=latents, scales=scales, A=A,
         hdr_illumination_colours=cols, illumination_directions=idirs, hdr_background_colours=bg,
         shape=np.array([R, S, D, NT, L]))


# ----------------------------------------------------------------------------- G11 field plumbing
def g11_field_outputs():
    g = gi.rng(11)
    R, S, GF, H = 6, 4, 16, 32
    o = g.uniform(-0.3, 0.3, (R, 3)).astype(np.float32)
    d = gi.unit(g.normal(size=(R, 3))).astype(np.float32)
    starts = np.sort(g.uniform(0.05, 1.0, (R, S, 1)), 1).astype(np.float32)
    geo_w1, geo_b1 = gi.seeded_linear(g, 24, 3, 1.0)
    geo_w2, geo_b2 = gi.seeded_linear(g, 1 + GF, 24, 0.5)
    in_dim = 3 + 36 + GF
    cw = [gi.seeded_linear(g, H, in_dim, 0.3), gi.seeded_linear(g, H, H, 0.3), gi.seeded_linear(g, 3, H, 0.3)]
    cg = [g.uniform(0.5, 1.5, (H, 1)).astype(np.float32), g.uniform(0.5, 1.5, (H, 1)).astype(np.float32),
          g.uniform(0.5, 1.5, (3, 1)).astype(np.float32)]

    def geo(x):  # stand-in for nerfstudio SDFField.forward_geonetwork (external)
        h = torch.nn.functional.softplus(x @ T(geo_w1).T + T(geo_b1), beta=100)
        return h @ T(geo_w2).T + T(geo_b2)

    self = NS(config=NS(geo_feat_dim=GF, predict_shininess=False), forward_geonetwork=geo,
              position_encoding=lambda x: nerf_encoding_standin(x, 6, 5.0, False), num_layers_color=4,
              relu=torch.nn.ReLU(), sigmoid=torch.nn.Sigmoid())
    for l, ((w, b), gg) in enumerate(zip(cw, cg)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        lin = torch.nn.utils.weight_norm(lin)  # sdf_albedo_field.py:159-160
        with torch.no_grad():
            lin.weight_v.copy_(T(w)); lin.weight_g.copy_(T(gg)); lin.bias.copy_(T(b))
        setattr(self, f"clin{l}", lin)
    self.get_colors = functools.partial(rsdf.SDFAlbedoField.get_colors, self)
    dirs_rs = T(d)[:, None, :].expand(R, S, 3).contiguous()
    pos = T(o)[:, None, :] + dirs_rs * T(starts)
    rs = Bag(camera_indices=torch.zeros(R, S, 1, dtype=torch.long),
             frustums=Bag(directions=dirs_rs, get_start_positions=lambda: pos.clone()))
    # neusky/fields/sdf_albedo_field.py:211-269 (+ get_colors :185-209)
    out = rsdf.SDFAlbedoField.get_outputs(self, rs, return_alphas=False)
    vals = list(out.values())  # insertion order: ALBEDO, SDF, NORMALS, GRADIENT (:253-260)
    save("g11_field_outputs", o=o, d=d, starts=starts, geo_w1=geo_w1, geo_b1=geo_b1, geo_w2=geo_w2, geo_b2=geo_b2,
         **{f"cw{i}": cw[i][0] for i in range(3)}, **{f"cb{i}": cw[i][1] for i in range(3)},
         **{f"cg{i}": cg[i] for i in range(3)},
         albedo=vals[0], sdf=vals[1], normals=vals[2], gradients=vals[3])


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    g1_srgb(); g2_sphere(); g3_lambertian(); g4_visibility(); g5_local_frame(); g6_ddf_field_and_model()
    g7_losses(); g8_film_siren(); g9_sample_illumination(); g11_field_outputs()
    assert not any("__pycache__" in r for r, _, _ in os.walk("/root/reference")), "bytecode leaked into reference"
