"""Proposal-network sampling.

Restates nerfstudio's ProposalNetworkSampler / UniformSampler / PDFSampler / HashMLPDensityField as the
reference drives them (`self.proposal_sampler(ray_bundle, density_fns=...)`, neusky/models/neusky_model.py:561;
sizes from NeuSFactoModelConfig).  The upstream source is not vendored in the
reference -> parity unpinned; this file is this project's definition, checked against oracle/.
Density = hash encode (HIP) -> 16-wide ReLU layer (MFMA GEMM) -> exp; re-sampling = nsky_pdf_sample.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .. import hip, ops
from ..encoding import HashGridGeometry
from ..fields.sdf_albedo_field import HashEncoding


class HashMLPDensityField(nn.Module):
    """nerfstudio HashMLPDensityField(num_layers=2, hidden_dim=16, num_levels=5, log2_hashmap_size=17, max_res=64|256)."""

    def __init__(self, hidden_dim: int = 16, num_levels: int = 5, max_res: int = 64, base_res: int = 16,
                 log2_hashmap_size: int = 17, contraction_mode: int = hip.MODE_CONTRACT_LINF):
        super().__init__()
        self.geom = HashGridGeometry(n_levels=num_levels, log2_hashmap_size=log2_hashmap_size, base_res=base_res,
                                     max_res=max_res, smoothstep=False)
        self.encoding = HashEncoding(self.geom)
        self.lin0 = nn.Linear(self.geom.out_dim, hidden_dim)
        self.lin1 = nn.Linear(hidden_dim, 1)
        self.mode = contraction_mode

    def invalidate_weight_cache(self) -> None:
        """once per optimisation step: the zero-padded copies of the two small layers are shared by every pass of the step"""
        self._wcache = {}

    def _padded(self):
        c = getattr(self, "_wcache", None)
        key = torch.is_grad_enabled()
        if c is not None and key in c:
            return c[key]
        w = (ops.pad_weight(self.lin0.weight), ops.pad_bias(self.lin0.bias), ops.pad_weight(self.lin1.weight), ops.pad_bias(self.lin1.bias))
        if c is not None:
            c[key] = w
        return w

    def raw_density(self, positions: torch.Tensor) -> torch.Tensor:
        """positions [R,n,3] -> pre-activation of the density head, [R*n, 4] (column 0; columns 1-3 are padding)"""
        x = positions.reshape(-1, 3).detach()
        feat = ops.HashEncodeFn.apply(x, self.encoding.table, self.geom, self.mode, False, 0, 0.0, False, False)
        if hip.proposal_mlp_supported(self.lin0.in_features, self.lin0.out_features) and self.lin1.out_features == 1:
            # both layers in registers, one kernel each way (csrc/proposal.hip) -> [R*n, 1]
            return ops.ProposalMLPFn.apply(feat, self.lin0.weight, self.lin0.bias, self.lin1.weight, self.lin1.bias)
        w0, b0, w1, b1 = self._padded()
        h = ops.DenseFn.apply(feat, w0, b0, self.lin0.out_features, "relu", True)
        return ops.DenseFn.apply(h, w1, b1, 1, "none", True)

    def density_fn(self, positions: torch.Tensor) -> torch.Tensor:
        """positions [R,n,3] -> density [R,n,1].  Under scene contraction every point maps strictly inside
        (0,1)^3, so nerfstudio's `selector` mask is identically one and is not materialised."""
        R, n, _ = positions.shape
        return ops.TruncExpFn.apply(self.raw_density(positions)[:, :1]).view(R, n, 1)

    def weights_fn(self, positions: torch.Tensor, ebins: torch.Tensor) -> torch.Tensor:
        """positions [R,n,3] (bin mid-points), ebins [R,n+1] -> volumetric weights [R,n]: density activation and
        `weights_from_density` fused into one launch each way (ops.DensityWeightsFn)"""
        return ops.DensityWeightsFn.apply(self.raw_density(positions), ebins)


def weights_from_density(density: torch.Tensor, deltas: torch.Tensor) -> torch.Tensor:
    """nerfstudio RaySamples.get_weights: density, deltas [R,n,1] -> weights [R,n,1]"""
    dd = deltas * density
    alphas = 1 - torch.exp(-dd)
    T = torch.cumsum(dd[..., :-1, :], dim=-2)
    T = torch.exp(-torch.cat([torch.zeros_like(dd[..., :1, :]), T], dim=-2))  # (dd, not T: with one bin T has no row to copy)
    return torch.nan_to_num(alphas * T)


class ProposalNetworkSampler(nn.Module):
    def __init__(self, num_nerf_samples_per_ray: int = 48, num_proposal_samples_per_ray: Tuple[int, ...] = (256, 96),
                 num_proposal_network_iterations: int = 2, histogram_padding: float = 0.01):
        super().__init__()
        self.num_nerf_samples_per_ray = num_nerf_samples_per_ray
        self.num_proposal_samples_per_ray = tuple(num_proposal_samples_per_ray)
        self.num_proposal_network_iterations = num_proposal_network_iterations
        self.histogram_padding = histogram_padding
        self._anneal = 1.0
        # device scalar mirror of _anneal: a captured graph reads it, so it is only ever written OUTSIDE a capture
        self.register_buffer("_anneal_t", torch.ones(1), persistent=False)
        self._u_cache: Dict[Tuple[int, bool, str], torch.Tensor] = {}

    def set_anneal(self, anneal: float) -> None:
        """nerfstudio's set_anneal callback.  The device mirror is NOT written while a HIP graph is being captured: a
        captured fill would bake the capture-time value into every replay and overwrite what the caller set before the
        replay (GraphedTrainStep.step writes it eagerly, then replays)."""
        self._anneal = anneal
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return
        self._anneal_t.fill_(anneal)

    def _u_base(self, num_bins: int, stratified: bool, device) -> torch.Tensor:
        key = (num_bins, stratified, str(device))
        if key not in self._u_cache:
            u = torch.linspace(0.0, 1.0 - (1.0 / num_bins), steps=num_bins)  # host linspace == the reference's
            if not stratified:
                u = u + 1.0 / (2 * num_bins)
            self._u_cache[key] = u.to(device)
        return self._u_cache[key]

    def forward(self, origins, directions, nears, fars, density_fns, jitters: Optional[Sequence[torch.Tensor]],
                want_inds: bool = False):
        """origins/directions [R,3], nears/fars [R,1]; jitters: one [R,1] uniform per level or None (eval).
        Returns final (sbins, ebins) [R,S+1], weights_list / sbins_list of the proposal levels, searchsorted inds."""
        n = self.num_proposal_network_iterations
        weights_list: List[torch.Tensor] = []
        sbins_list: List[torch.Tensor] = []
        inds_list: List[torch.Tensor] = []
        sbins = ebins = weights = None
        for lvl in range(n + 1):
            ns = self.num_proposal_samples_per_ray[lvl] if lvl < n else self.num_nerf_samples_per_ray
            jit = None if jitters is None else jitters[lvl]
            o_c, d_c = origins.detach().contiguous(), directions.detach().contiguous()
            if lvl == 0:
                sbins, ebins = hip.uniform_bins(nears, fars, ns, None if jit is None else jit.reshape(-1).contiguous())
            else:
                annealed = torch.pow(weights.detach(), self._anneal_t)  # tensor exponent: the value can change under a captured graph
                sbins, inds = hip.pdf_sample(annealed.contiguous(), sbins, self._u_base(ns + 1, jit is not None, sbins.device),
                                             None if jit is None else jit.reshape(-1).contiguous(), ns + 1,
                                             self.histogram_padding, 1e-5, want_inds)
                inds_list.append(inds)
            if lvl < n:
                # euclidean bins (levels > 0) and the bin mid-points along the ray in one launch
                e_new, pos = hip.bins_to_samples(sbins, nears, fars, o_c, d_c, want_ebins=lvl > 0, want_positions=True)
                ebins = e_new if lvl > 0 else ebins
                owner = getattr(density_fns[lvl], "__self__", None)
                if isinstance(owner, HashMLPDensityField):  # this package's proposal field: fused density -> weights
                    weights = owner.weights_fn(pos, ebins)
                else:  # any other density callable (nerfstudio's `density_fns` contract)
                    dens = density_fns[lvl](pos)
                    weights = weights_from_density(dens, (ebins[:, 1:] - ebins[:, :-1])[..., None])[..., 0]
                weights_list.append(weights)
                sbins_list.append(sbins)
            else:
                ebins, _ = hip.bins_to_samples(sbins, nears, fars)
        return sbins, ebins, weights_list, sbins_list, inds_list
