"""The scene the frame tests share: a small randomised pipeline in eval mode and the rays of one camera's H x W frame."""
import torch

from util_step import randomise, small_pipeline_config


def frame_scene(H, W, device, seed=0):
    """-> (pipe, rb): small_pipeline_config(R=16, D=32, images=4) set up under torch.manual_seed(seed) and randomised, its
    eval latents and scales drawn from generator seed 3, in eval mode; rb: H x W rays from generator seed 5, all from the first
    ray's origin (one camera), with camera index 1"""
    torch.manual_seed(seed)
    pipe = small_pipeline_config(R=16, D=32, images=4).setup(device=device)
    randomise(pipe)
    m = pipe.model
    with torch.no_grad():
        g = torch.Generator().manual_seed(3)
        m.eval_illumination_latents.copy_((torch.randn(m.eval_illumination_latents.shape, generator=g) * 0.3).to(device))
        m.eval_scale.copy_((1 + 0.2 * torch.rand(m.eval_scale.shape, generator=g)).to(device))
    pipe.eval()
    rb, _ = pipe.datamanager._rays(H * W, torch.Generator().manual_seed(5))
    rb.origins = rb.origins[:1].expand(H * W, 3).contiguous().view(H, W, 3)  # one camera
    rb.directions = rb.directions.view(H, W, 3)
    rb.camera_indices = torch.ones(H, W, 1, dtype=torch.long, device=device)
    rb.pixel_area = rb.pixel_area.view(H, W, 1)
    rb.metadata = {"directions_norm": torch.ones(H, W, 1, device=device)}
    return pipe, rb
