"""Pack direction 3 of the FiLM chain (csrc/film_chain.hip: the weight stream of the backward on saved operands) on the host: the tile
count and stream length nsky_film_stream_layout reports against the layout comment -- direction 1 without its two tiles (F, phase) per
32 features and FiLM layer: (n_film - 1) hidden / 32 transposed tiles, then the layer-0 input tile, every tile a whole number of
16 KB groups.  No GPU: the layout is host arithmetic over a descriptor whose pointers are never followed.  (The order and the bytes of
the packed tiles are the GPU test's round trip, tests/test_gpu_film_saved_operands.py.)"""
import pytest

GROUP, RING_GROUPS = 16384, 8


def _descriptor(H, n_map, n_film, cond_dim, x_dim, out_dim):
    """the network's geometry with placeholder addresses: the layout reads the sizes and checks the pointers for NULL only"""
    from neusky_amd import hip
    d = hip.FilmNet(hidden=H, n_map=n_map, n_film=n_film, cond_dim=cond_dim, x_dim=x_dim, out_dim=out_dim)
    for l in range(n_map):
        d.map_w[l], d.map_b[l], d.map_ld[l] = 16, 16, (cond_dim + 3) // 4 * 4 if l == 0 else H
    for i in range(n_film):
        d.film_w[i], d.film_b[i], d.film_ld[i] = 16, 16, (x_dim + 3) // 4 * 4 if i == 0 else H
    d.mo_w, d.mo_b, d.mo_ld = 16, 16, H
    d.out_w, d.out_b, d.out_ld = 16, 16, H
    return d


@pytest.mark.parametrize("net", [(128, 1, 1, 1, 1, 1), (256, 2, 1, 300, 16, 3), (128, 5, 9, 300, 10, 3), (256, 5, 5, 35, 15, 1), (128, 3, 12, 36, 8, 2)])
def test_direction_3_tile_count_and_stream_bytes(net):
    from neusky_amd import hip
    H, n_map, n_film = net[:3]
    d = _descriptor(*net)
    NT, Gh = H // 32, (H // 16 + 7) // 8
    bytes1, tiles1 = hip.film_stream_layout(d, 1)
    bytes3, tiles3 = hip.film_stream_layout(d, 3)
    assert tiles3 == (n_film - 1) * NT + 1
    assert tiles1 - tiles3 == 2 * n_film * NT, "direction 1's F and phase tiles"
    # every tile Gh groups; the ring's read-ahead (RING_GROUPS + 2 groups) behind the last one, as in every direction
    assert bytes3 == (tiles3 * Gh + RING_GROUPS + 2) * GROUP
    assert bytes1 - bytes3 == 2 * n_film * NT * Gh * GROUP


def test_direction_4_is_refused():
    from neusky_amd import hip
    d = _descriptor(128, 1, 1, 1, 1, 1)
    with pytest.raises(hip.NeuSkyHipError):
        hip.film_stream_layout(d, 4)
