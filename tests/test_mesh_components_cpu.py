"""Mesh components and floater removal, the parts that need no GPU: the numpy restatement (tests/mesh_components_cpu.py) on hand-made
meshes and on a marching-cubes mesh, and the host logic of neusky_amd.exporter.components (argument checks, the command line's flags)."""
import numpy as np
import pytest
import torch

import marching_cubes_cpu as M
import mesh_components_cpu as CC

TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]])


def test_two_tetrahedra_and_a_loose_vertex():
    faces = np.concatenate([TETRA + 5, TETRA])  # vertices 0-3 and 5-8; vertex 4 has no face
    out = CC.label_components_cpu(9, faces)
    assert out["roots"].tolist() == [0, 5] and out["face_counts"].tolist() == [4, 4]  # the tie in size goes to the smaller root
    assert out["labels"].tolist() == [0, 0, 0, 0, -1, 1, 1, 1, 1]
    assert out["face_labels"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    assert out["labels"].dtype == np.int32 and out["face_counts"].dtype == np.int64


def test_a_pinch_point_joins_two_bodies():
    faces = np.concatenate([TETRA, TETRA + 3])  # vertex 3 belongs to both
    out = CC.label_components_cpu(7, faces)
    assert out["roots"].tolist() == [0] and out["face_counts"].tolist() == [8]
    assert (out["labels"] == 0).all() and (out["face_labels"] == 0).all()
    apart = np.concatenate([TETRA, TETRA + 4])  # the same positions could be given twice: indices decide, not positions
    assert CC.label_components_cpu(8, apart)["roots"].tolist() == [0, 4]


def test_rank_is_by_size_then_root_and_ignores_face_order():
    strip = np.array([[i, i + 1, i + 2] for i in range(10, 16)])  # 6 faces, root 10
    faces = np.concatenate([TETRA + 20, strip, TETRA + 2, [[30, 31, 32]]])
    out = CC.label_components_cpu(33, faces)
    assert out["roots"].tolist() == [10, 2, 20, 30] and out["face_counts"].tolist() == [6, 4, 4, 1]
    perm = np.random.default_rng(0).permutation(len(faces))
    again = CC.label_components_cpu(33, faces[perm][:, [1, 2, 0]])
    assert np.array_equal(again["labels"], out["labels"]) and np.array_equal(again["roots"], out["roots"])
    assert np.array_equal(again["face_labels"], out["face_labels"][perm])
    assert (out["labels"][[0, 1, 6, 7, 8, 9, 18, 19]] == -1).all()


@pytest.mark.parametrize("order", ["identity", "reversed", "random"])
def test_a_long_strip_is_one_component(order):
    n = 3000
    number = {"identity": np.arange(n + 2), "reversed": np.arange(n + 2)[::-1], "random": np.random.default_rng(1).permutation(n + 2)}[order]
    faces = number[np.stack([np.arange(n), np.arange(n) + 1, np.arange(n) + 2], 1)]
    out = CC.label_components_cpu(n + 2, faces)
    assert out["roots"].tolist() == [0] and out["face_counts"].tolist() == [n] and (out["labels"] == 0).all()


def test_filtering_keeps_order_orientation_and_attribute_rows():
    strip = np.array([[i, i + 1, i + 2] for i in range(10, 16)])
    faces = np.concatenate([TETRA + 20, strip, TETRA + 2, [[30, 31, 32]]])
    rng = np.random.default_rng(2)
    v = rng.standard_normal((33, 3)).astype(np.float32)
    c = rng.integers(0, 256, (33, 3)).astype(np.uint8)
    out = CC.remove_floaters_cpu(v, faces, keep_largest=2, colours=c)
    assert out["kept_components"] == 2 and len(out["faces"]) == 10 and len(out["vertices"]) == 4 + 8
    assert np.array_equal(out["vertices"][out["faces"]], v[np.concatenate([strip, TETRA + 2])])  # same corners, same order
    assert np.array_equal(out["colours"], c[np.r_[2:6, 10:18]])
    assert len(CC.remove_floaters_cpu(v, faces, min_faces=4)["faces"]) == 14
    assert len(CC.remove_floaters_cpu(v, faces, min_faces=5)["faces"]) == 6
    both = CC.remove_floaters_cpu(v, faces, keep_largest=3, min_faces=5)  # a component has to meet both
    assert both["kept_components"] == 1 and len(both["faces"]) == 6
    none = CC.remove_floaters_cpu(v, faces, min_faces=7)
    assert none["faces"].shape == (0, 3) and none["vertices"].shape == (0, 3)


def test_marching_cubes_spheres_are_separate_components():
    x = np.linspace(-1.0, 1.0, 24)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    vol = np.minimum(np.sqrt((X + 0.45) ** 2 + Y**2 + Z**2) - 0.35, np.sqrt((X - 0.55) ** 2 + Y**2 + Z**2) - 0.2).astype(np.float32)
    v, f = M.marching_cubes_cpu(vol, 0.0)
    out = CC.label_components_cpu(len(v), f)
    assert len(out["roots"]) == 2 and out["face_counts"][0] > out["face_counts"][1] > 0 and out["face_counts"].sum() == len(f)
    assert (out["labels"] >= 0).all()  # marching cubes emits no vertex without a face
    big = v[out["labels"] == 0]
    assert np.abs(np.linalg.norm(big + [0.45, 0, 0], axis=1) - 0.35).max() < 0.05  # rank 0 is the larger sphere


# ---- host logic of neusky_amd.exporter.components

def test_remove_floaters_is_exported_and_checks_its_arguments():
    from neusky_amd.exporter import Mesh, MeshComponents, label_components, remove_floaters
    assert MeshComponents.__dataclass_fields__.keys() == {"labels", "face_labels", "roots", "face_counts", "num_components"}
    host = Mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="at least one"):
        remove_floaters(host)
    for bad in (0, -3, 2.0, True, "2"):
        with pytest.raises(ValueError, match="keep_largest"):
            remove_floaters(host, keep_largest=bad)
        with pytest.raises(ValueError, match="min_faces"):
            remove_floaters(host, min_faces=bad)
    with pytest.raises(ValueError, match="min_faces"):
        remove_floaters(host, keep_largest=1, min_faces=0)
    with pytest.raises(ValueError, match="CUDA"):  # the kernels run on the device only: no host path
        remove_floaters(host, keep_largest=1)
    with pytest.raises(ValueError, match="CUDA"):
        label_components(host)


def test_cli_flags_exist_combine_and_default_off():
    from neusky_amd.exporter.__main__ import build_parser
    base = ["--checkpoint", "c.ckpt", "--output", "m.ply"]
    args = build_parser().parse_args(base)
    assert args.keep_largest_components is None and args.min_component_faces is None
    args = build_parser().parse_args(base + ["--keep-largest-components", "3", "--min-component-faces", "500", "--target-num-faces", "9"])
    assert args.keep_largest_components == 3 and args.min_component_faces == 500 and args.target_num_faces == 9
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--keep-largest-components", "1.5"])


@pytest.mark.parametrize("flag", ["--keep-largest-components", "--min-component-faces"])
@pytest.mark.parametrize("value", ["0", "-2"])
def test_cli_rejects_values_below_one_before_any_work(flag, value, capsys):
    from neusky_amd.exporter.__main__ import main
    with pytest.raises(SystemExit) as e:
        main(["--checkpoint", "does-not-exist.ckpt", "--output", "m.ply", flag, value])
    assert e.value.code == 2
    assert f"{flag} must be >= 1" in capsys.readouterr().err
