"""One train step of the small pipeline of test_gpu_step.py with the DDF-fit ground-truth pass in its directional form
(model config ddf_fit_directional, the default) and in the full quad form, from the same seeds and injected randoms: every loss
term and every parameter gradient of the two runs agree within the bars test_gpu_step.py holds HIP to against the oracle (2e-4 per
loss term, GRAD_BARS per tensor, of the quad run's largest entry), and the directional run's fit pass allocates two row-sets per
point."""
import pytest
import torch

from test_gpu_step import GRAD_BARS, _module_grads
from util_step import make_randoms, randomise, randoms_to, small_pipeline_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 16


def _step(directional, monkeypatch):
    from neusky_amd import hip
    torch.manual_seed(0)
    pipe = small_pipeline_config(R=R).setup(device=DEV)
    pipe.train()
    randomise(pipe)
    pipe.model.config.ddf_fit_directional = directional
    rb, batch = pipe.datamanager.next_train(0)
    rnd = make_randoms(pipe, R)
    pipe.model.set_step(10_000)
    for p in pipe.parameters():
        p.grad = None
    pair_calls = []
    real = hip.field_geo_fwd_dir

    def spy(net, pack, ET, N, a0q, *rest, **kw):
        pair_calls.append((N, a0q.shape[0], ET.shape[0]))
        return real(net, pack, ET, N, a0q, *rest, **kw)

    monkeypatch.setattr(hip, "field_geo_fwd_dir", spy)
    outs, loss_dict, _ = pipe.get_train_loss_dict(10_000, ray_bundle=rb, batch=batch, randoms=randoms_to(rnd, DEV))
    sum(loss_dict.values()).backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(hip, "field_geo_fwd_dir", real)
    grads = {k: v.detach().clone() for k, v in _module_grads(pipe).items() if v is not None}
    n_fit = rnd["ddf_rays"][0].shape[0] * pipe.model.config.num_neus_samples_per_ray
    return {k: float(v) for k, v in loss_dict.items()}, grads, pair_calls, n_fit


def test_directional_fit_pass_leaves_the_step_where_it_was(monkeypatch):
    from neusky_amd import hip
    loss_q, grads_q, calls_q, n_fit = _step(False, monkeypatch)
    loss_d, grads_d, calls_d, _ = _step(True, monkeypatch)
    assert calls_q == [], "switch off: the quad form"
    # switch on: ONE pair-layout pass, over the fit rays' samples, with two row-sets per point
    assert calls_d == [(n_fit, hip.film_rows(2 * n_fit), 2 * n_fit)], (calls_d, n_fit)
    assert sorted(loss_q) == sorted(loss_d)
    for k, b in loss_q.items():
        a = loss_d[k]
        print(f"{k}: quad {b:.9g} directional {a:.9g}")
        assert abs(a - b) < 2e-4 * max(abs(b), 1e-3), (k, a, b)
    net_of = lambda k: ("ddf.table" if k == "ddf.table" else k.split("_")[0]) if k.startswith("ddf.") else k.split(".")[0].split("_")[0]  # noqa: E731
    assert sorted(grads_q) == sorted(grads_d)
    bad = []
    for k, b in grads_q.items():
        a = grads_d[k]
        scale = b.abs().max().item() + 1e-30
        e = (a.double() - b.double()).abs().max().item() / scale
        print(f"{k}: {e:.3e} of the largest entry (bar {GRAD_BARS[net_of(k)]:.0e})")
        if e > GRAD_BARS[net_of(k)]:
            bad.append((k, e))
    assert not bad, bad
