"""CPU: the host side of cmflow_amd/results.py -- the numpy restatement of the pose chain against a straight matrix chain, the
reference's ``save_res`` layout against a file the reference itself wrote, the folder rule, merge / all_reduce, signatures, and the
refusal of CPU tensors.  The device code is tested in tests/test_gpu_results.py."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import results_ref as ref
from cmflow_amd import dataset as D
from cmflow_amd import evaluate as EV
from cmflow_amd import results as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _item(n1, n2, rng):
    r = lambda *s: rng.standard_normal(s).astype(np.float32)
    return (r(n1, 3), r(n2, 3), r(n1, 3), r(n2, 3), r(4, 4), r(n1, 3), (rng.random(n1) < 0.5).astype(np.float32), 0.1, r(n1), r(n1), r(n1, 2))


def _filled(n1s, n2s, batches, clips=None, seed=3):
    """A CPU split and the store a collector would have left after ``batches`` (lists of frame ids), filled by results_ref.pack from
    random network outputs; also those outputs per frame."""
    rng = np.random.default_rng(seed)
    items = [_item(a, b, rng) for a, b in zip(n1s, n2s)]
    split = D.DeviceSplit.from_items(items, "cpu", clips)
    res = R.SplitResults.empty(split)
    off1 = split.off1.numpy()
    store = {"flow": res.flow.numpy(), "score": res.score.numpy(), "mask": res.mask.numpy(), "pred_trans": res.pred_trans.numpy(),
             "gt_trans": res.gt_trans.numpy(), "done": res.done.numpy()}                   # views: pack fills the tensors
    outs = {}
    for frames in batches:
        nmax = max(n1s[f] for f in frames)
        sf = rng.standard_normal((len(frames), 3, nmax)).astype(np.float32)
        cls = rng.random((len(frames), nmax)).astype(np.float32)
        mk = (cls > 0.5).astype(np.uint8)
        pt = rng.standard_normal((len(frames), 4, 4)).astype(np.float32)
        gt = np.stack([items[f][4] for f in frames])
        ref.pack(store, off1, frames, [n1s[f] for f in frames], sf, cls, mk, pt, gt)
        for s, f in enumerate(frames):
            outs[f] = (sf[s, :, :n1s[f]], mk[s, :n1s[f]], pt[s])
    return items, split, res, outs


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
def _bound(L, P):
    return 16 * L * 2.0 ** -53 * max(1.0, float(np.abs(P).max()))


def test_chain_restatement_equals_a_straight_inverse_and_matmul_chain():
    """Rotations that are exactly orthonormal in float32 (signed permutations, i.e. quarter turns) with random translations: the
    rigid inverse IS the matrix inverse, so the elementwise restatement must agree with np.linalg.inv / @ to the rounding of L
    successive 4x4 products, 16 L 2^-53 max(1, max|P|)."""
    rng = np.random.default_rng(0)
    L = 65
    T = np.zeros((L, 4, 4), dtype=np.float32)
    for k in range(L):
        perm, sign = rng.permutation(3), rng.choice([-1.0, 1.0], 3)
        T[k, np.arange(3), perm] = sign
        T[k, :3, 3] = rng.standard_normal(3)
        T[k, 3, 3] = 1
    clips = [(0, 1), (1, 3), (3, 3), (5, L)]
    got, want = ref.pose_chain(T, clips), ref.pose_chain_linalg(T, clips, inverse=np.linalg.inv)
    assert np.isnan(got[3:5]).all() and np.isnan(want[3:5]).all()
    inside = [k for a, b in clips for k in range(a, b)]
    err = np.abs(got[inside] - want[inside]).max()
    print("chain vs np.linalg.inv chain: max err %.3g, bound %.3g" % (err, _bound(L, want[inside])))
    assert err <= _bound(L, want[inside])
    assert (got[inside][:, 3] == (0, 0, 0, 1)).all()


def test_chain_restatement_on_the_saved_sequence():
    """The reference's own 337 saved transforms of delft_12 (rotations off orthonormal by about 1e-3, so the chain is defined with the
    rigid inverse of odometry_util.se3_inverse, not the matrix inverse): elementwise restatement against ``@`` with that inverse,
    same bound."""
    T = np.load(os.path.join(GOLDEN, "saved_pred_t_delft_12.npz"))["pred_t"]
    assert T.shape == (337, 4, 4) and T.dtype == np.float32
    R3 = T[:, :3, :3].astype(np.float64)
    off = np.abs(R3 @ R3.transpose(0, 2, 1) - np.eye(3)).max()
    assert 1e-5 < off < 5e-3, off                                                       # the realistic input: not orthonormal
    got, want = ref.pose_chain(T, [(0, 337)]), ref.pose_chain_linalg(T, [(0, 337)])
    err = np.abs(got - want).max()
    print("saved sequence: max|P| %.3g, max err %.3g, bound %.3g" % (np.abs(want).max(), err, _bound(337, want)))
    assert err <= _bound(337, want)


# ---- the reference's files -----------------------------------------------------------------------------------------------------------
def _depth(x):
    return 1 + _depth(x[0]) if isinstance(x, list) else 0


def _leaf_types(x):
    return set().union(*(_leaf_types(v) for v in x)) if isinstance(x, list) else {type(x)}


def test_write_json_has_the_layout_of_a_file_the_reference_wrote(tmp_path):
    """tests/golden/save_res_frame.json is delft_12/1000.json of the reference's saved results cut to 8 points per array.  A store
    holding exactly that frame must come back out with the same keys, nesting, element types -- and values."""
    want = json.load(open(os.path.join(GOLDEN, "save_res_frame.json")))
    f32 = lambda v: np.array(v, dtype=np.float32)
    pc1, pc2 = f32(want["pc1"]).T, f32(want["pc2"]).T
    n1, n2 = pc1.shape[0], pc2.shape[0]
    z = np.zeros
    item = (pc1, pc2, z((n1, 3)), z((n2, 3)), np.eye(4), z((n1, 3)), z(n1), 0.1, z(n1), z(n1), z((n1, 2)))
    split = D.DeviceSplit.from_items([item], "cpu")
    res = R.SplitResults.empty(split)
    res.flow.copy_(torch.from_numpy(f32(want["pred_f"]).T.copy()))
    res.mask.copy_(torch.from_numpy(np.array(want["pred_m"]).astype(np.uint8)))
    res.pred_trans[0] = torch.from_numpy(f32(want["pred_t"]))
    with pytest.raises(ValueError):
        res.write_json(str(tmp_path / "early"), split)                                  # not done
    assert not (tmp_path / "early").exists()
    res.done.fill_(1)
    paths = res.write_json(str(tmp_path), split, clip_names=["delft_12"])
    assert paths == [str(tmp_path / "delft_12" / "0.json")]
    got = json.load(open(paths[0]))
    assert list(got) == list(want) == ["pc1", "pc2", "pred_f", "pred_m", "pred_t"]
    for k in want:
        assert _depth(got[k]) == _depth(want[k]), k
        assert _leaf_types(got[k]) == _leaf_types(want[k]) == {float}, k
        assert np.array(got[k]).shape == np.array(want[k]).shape, k
    assert got == want


N1S, N2S = (5, 1, 9, 4, 7, 3, 6), (8, 9, 8, 12, 10, 9, 11)


@pytest.mark.parametrize("batches", [[[0, 1, 2], [3, 4, 5, 6]], [[0, 1], [2, 3], [4, 5], [6]], [[6, 2, 4], [1, 5], [3, 0]]])
def test_folders_switch_where_the_reference_switches(tmp_path, batches):
    """Clips [(0,3),(3,7)]: frames 0-2 in the first folder, 3-6 in the second under their GLOBAL index -- whether the boundary falls
    between two batches, inside a batch ([2,3]) or the batches are out of order; content = the outputs of the frame."""
    _, split, res, outs = _filled(N1S, N2S, batches, clips=[(0, 3), (3, 7)])
    paths = res.write_json(str(tmp_path), split, clip_names=["delft_a", "delft_b"])
    assert [os.path.relpath(p, str(tmp_path)) for p in paths] == ["delft_a/%d.json" % i for i in range(3)] + ["delft_b/%d.json" % i for i in range(3, 7)]
    assert sorted(os.listdir(str(tmp_path))) == ["delft_a", "delft_b"]
    for i, p in enumerate(paths):
        got = json.load(open(p))
        sf, mk, pt = outs[i]
        assert got["pred_f"] == sf.tolist() and got["pred_m"] == mk.astype(float).tolist() and got["pred_t"] == pt.astype(float).tolist()
        a, b = int(split.off1[i]), int(split.off1[i + 1])
        assert got["pc1"] == split.tab1[a:b, :3].T.tolist() and np.array(got["pc2"]).shape == (3, N2S[i])
    # without clip ranges: one folder; default names
    _, split1, res1, _ = _filled(N1S, N2S, batches)
    one = res1.write_json(str(tmp_path / "plain"), split1)
    assert [os.path.relpath(p, str(tmp_path / "plain")) for p in one] == ["clip_0/%d.json" % i for i in range(7)]
    with pytest.raises(ValueError):
        res.write_json(str(tmp_path / "bad"), split, clip_names=["only_one"])


# ---- combining -----------------------------------------------------------------------------------------------------------------------
def _equal(a, b):
    return all(torch.equal(getattr(a, k).nan_to_num(nan=-7.0) if k == "metrics" else getattr(a, k),
                           getattr(b, k).nan_to_num(nan=-7.0) if k == "metrics" else getattr(b, k)) for k in R._FIELDS) and a.clips == b.clips


def _with_metrics(res, rng):
    done = res.done.bool()
    res.metrics[done] = torch.from_numpy(rng.standard_normal((int(done.sum()), 14)))
    return res


def test_merge_takes_each_frame_from_the_side_that_has_it():
    rng = np.random.default_rng(5)
    _, _, whole, _ = _filled(N1S, N2S, [[0, 1, 2, 3, 4, 5, 6]])
    _, _, a, _ = _filled(N1S, N2S, [[0, 1, 2, 3, 4, 5, 6]])
    _with_metrics(whole, rng)
    whole.metrics[2, 3] = float("nan")                                                  # a NaN metric of an evaluated frame
    a.metrics.copy_(whole.metrics)
    assert _equal(a, whole)
    parts = []
    for mine in ([0, 2, 5], [1, 3, 4, 6]):
        _, _, p, _ = _filled(N1S, N2S, [[0, 1, 2, 3, 4, 5, 6]])                         # same seed: same outputs
        keep = torch.zeros(7, dtype=torch.bool)
        keep[mine] = True
        rows = torch.repeat_interleave(keep, torch.tensor(N1S))
        p.flow[~rows], p.score[~rows], p.mask[~rows] = 0, 0, 0
        p.pred_trans[~keep], p.gt_trans[~keep], p.done[~keep] = 0, 0, 0
        p.metrics.copy_(torch.where(keep[:, None], whole.metrics, torch.full_like(whole.metrics, float("nan"))))
        parts.append(p)
    merged = parts[0].merge(parts[1])
    assert _equal(merged, whole) and merged is not parts[0]
    assert _equal(parts[1].merge(parts[0]), whole)
    with pytest.raises(ValueError, match="done in both"):
        merged.merge(parts[1])                                                          # frames 1, 3, 4, 6 on both sides
    _, _, other, _ = _filled(N1S[:-1], N2S[:-1], [[0]])
    with pytest.raises(ValueError):
        parts[0].merge(other)                                                           # another split


def test_all_reduce_sums_disjoint_parts_and_keeps_nan_where_nobody_wrote(monkeypatch):
    """The rule of SplitResults.all_reduce with the collective replaced by an addition of the other rank's tensors: rows of frames
    nobody evaluated stay NaN, an evaluated frame's NaN metric stays NaN, everything else is the owner's value."""
    rng = np.random.default_rng(6)
    _, _, a, _ = _filled(N1S, N2S, [[0, 2, 5]], seed=1)
    _, _, b, _ = _filled(N1S, N2S, [[1, 3, 6]], seed=2)                                 # frame 4: nobody
    _with_metrics(a, rng), _with_metrics(b, rng)
    a.metrics[2, 3] = float("nan")
    want = a.merge(b)
    theirs = [b.flow, b.score, b.mask, b.pred_trans, b.gt_trans, torch.where(b.done.bool()[:, None], b.metrics, torch.zeros_like(b.metrics)), b.done]
    peers = iter(theirs)
    monkeypatch.setattr(R.dist, "all_reduce", lambda t, op=None, group=None: t.add_(next(peers)))
    assert a.all_reduce() is a
    assert _equal(a, want)
    assert torch.isnan(a.metrics[4]).all() and torch.isnan(a.metrics[2, 3]) and a.done.tolist() == [1, 1, 1, 1, 0, 1, 1]


def test_frame_per_frame_worst_save_load(tmp_path):
    rng = np.random.default_rng(8)
    _, split, res, outs = _filled(N1S, N2S, [[3, 0, 6], [1, 2, 4]], clips=[(0, 3), (3, 7)])         # frame 5 missing
    _with_metrics(res, rng)
    for f, (sf, mk, pt) in outs.items():
        fr = res.frame(f)
        assert np.array_equal(fr["flow"].numpy(), sf.T) and np.array_equal(fr["mask"].numpy(), mk) and np.array_equal(fr["pred_trans"].numpy(), pt)
        assert fr["score"].shape == (N1S[f],) and int(fr["done"]) == 1 and fr["metrics"].shape == (14,)
    assert int(res.frame(5)["done"]) == 0 and not res.frame(5)["flow"].any() and torch.isnan(res.frame(5)["metrics"]).all()
    with pytest.raises(IndexError):
        res.frame(7)
    assert R.METRIC_KEYS == EV.METRIC_KEYS and len(R.METRIC_KEYS) == 14
    epe = res.per_frame("epe")
    assert epe.shape == (7,) and torch.equal(epe[:5], res.metrics[:5, R.METRIC_KEYS.index("epe")])
    with pytest.raises(KeyError):
        res.per_frame("EPE")
    vals, idx = res.worst("epe", 7)
    order = sorted((f for f in range(7) if f != 5), key=lambda f: -float(epe[f]))
    assert idx.tolist() == order + [5] and torch.isnan(vals[-1]) and torch.equal(vals[:6], epe[order])
    vals, idx = res.worst("acc", 3, largest=False)
    acc = res.per_frame("acc")
    assert idx.tolist() == sorted((f for f in range(7) if f != 5), key=lambda f: float(acc[f]))[:3]
    with pytest.raises(ValueError):
        res.worst("epe", 8)
    path = str(tmp_path / "res.pt")
    res.save(path)
    back = R.SplitResults.load(path, "cpu")
    assert _equal(back, res) and back.clips == [(0, 3), (3, 7)] and os.listdir(str(tmp_path)) == ["res.pt"]
    split.save(str(tmp_path / "split.pt"))
    with pytest.raises(ValueError):
        R.SplitResults.load(str(tmp_path / "split.pt"), "cpu")                          # a DeviceSplit file


# ---- interface -----------------------------------------------------------------------------------------------------------------------
def test_public_signatures():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(EV.test_split) == sig(EV.eval_split)
    assert sig(EV.test_split_clips) == sig(EV.eval_split_clips)
    assert sig(R.ResultCollector.__init__) == ["self", "split", "args"] and sig(R.ResultCollector.__call__) == ["self", "batch", "outputs"]
    assert inspect.signature(R.ResultCollector.__init__).parameters["args"].default is None
    assert sig(R.SplitResults.write_json) == ["self", "directory", "split", "clip_names"]
    assert sig(R.SplitResults.trajectories) == ["self", "which"] and inspect.signature(R.SplitResults.trajectories).parameters["which"].default == "pred"
    assert inspect.signature(R.SplitResults.odometry_metrics).parameters["deltas"].default == (1, 10)
    for name in ("frame", "per_frame", "worst", "merge", "all_reduce", "save", "load", "empty"):
        assert callable(getattr(R.SplitResults, name)), name
    assert not getattr(EV.test_split, "__test__", True) and not getattr(EV.test_split_clips, "__test__", True)
    from cmflow_amd import _lib
    for name in ("cmf_pack_results", "cmf_eval_metrics_frames", "cmf_pose_chain"):
        assert name in _lib.SIGNATURES, name


def test_cpu_tensors_are_refused(args):
    """No CPU fallback: filling a store and chaining poses need the GPU, and say so before anything is launched."""
    from cmflow_amd.cmflow import CMFlow
    from cmflow_amd.raflow import RaFlow
    _, split, res, _ = _filled(N1S, N2S, [[0, 1, 2, 3, 4, 5, 6]])
    with pytest.raises(RuntimeError, match="GPU"):
        R.ResultCollector(split)
    with pytest.raises(RuntimeError, match="GPU"):
        res.trajectories()
    with pytest.raises(RuntimeError, match="GPU"):
        res.odometry_metrics()
    with pytest.raises(ValueError):
        res.trajectories("both")
    net = CMFlow(args)
    net.train()
    with pytest.raises(RuntimeError, match="GPU"):
        EV.test_split(net, split, 4)
    with pytest.raises(ValueError):
        EV.test_split_clips(net, split, 4, 2)                                           # CMFlow is not CMFlow_T
    class A:
        num_points, stat_thres, rigid_thres = 256, 0.5, 0.15
    with pytest.raises(NotImplementedError):
        EV.test_split(RaFlow(A()), split, 4)
    assert net.training                                                                 # every refusal comes before net.eval()


def test_pose_chain_has_no_contracted_arithmetic():
    """The chain is a definition with every operation rounded on its own: the kernel's code must hold no fused multiply-add."""
    import re
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(repo, "cmflow_amd", "csrc", "results.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", "-", src],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    asm = out.stdout
    start = asm.index("pose_chain_kernel")
    body = asm[start:asm.index("s_endpgm", start)]
    assert re.search(r"v_mul_f64", body) and re.search(r"v_add_f64", body)
    assert not re.search(r"v_(fma|fmac|mad|pk_fma)_f64", body)
