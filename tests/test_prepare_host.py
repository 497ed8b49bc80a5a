"""CPU: the host side of cmflow_amd/prepare.py -- ``match_boxes`` against the restatement (tests/prepare_ref.py), every argument
error (ValueError, before anything is launched) and the refusal to run without a GPU (RuntimeError)."""
import numpy as np
import pytest
import torch

import prepare_case as PC
import prepare_ref as R
from cmflow_amd import prepare as P
from prepare_case import product_calib


@pytest.mark.parametrize("per_scan", [False, True])
def test_match_boxes_is_the_restatements_matching(per_scan):
    case = PC.chain(11, [120, 150, 90], "gt", K=7, per_scan_calib=per_scan)
    calib = product_calib(case)
    assert (calib.per_scan == 3) if per_scan else (calib.per_scan is None)
    total = 0
    for a, b in case.pairs:
        got = P.match_boxes(case.tracks[a], case.tracks[b], calib.scan(a), calib.scan(b))
        want = R.matched_boxes(case.tracks[a], case.tracks[b], case.calib[a], case.calib[b])
        assert got.shape == (len(want), P.BOX_DOUBLES) and got.dtype == np.float64
        for rec, ((c1, r1, ext), (c2, r2, _), score) in zip(got, want):
            t12 = np.dot(R.box_pose(r2, c2), np.linalg.inv(R.box_pose(r1, c1)))
            # float64 on coordinates below 400 m over a dozen operations: 1e-12 leaves three decades
            np.testing.assert_allclose(rec, np.concatenate([c1, r1.reshape(9), ext / 2, t12.reshape(16), [score]]), rtol=0, atol=1e-12)
        total += len(want)
    assert total >= 8                                                      # kinds 0, 2, 3, 4 of the own boxes and the far one, twice
    # the first-match rule and the skipped rows, on ids alone
    l1, l2 = case.tracks[1], case.tracks[2]
    ids = [r[-1] for r in l1 if (l2[:, -1] == r[-1]).any()]
    assert [r[-1] for r in l1 if r[-1] not in ids] != [] and len(ids) == len(P.match_boxes(l1, l2, calib.scan(1), calib.scan(2)))
    dup = [i for i in ids if (l2[:, -1] == i).sum() == 2]
    assert dup                                                             # kind 2: twice in frame 2
    first = l2[np.where(l2[:, -1] == dup[0])[0][0]]
    rec = P.match_boxes(l1[l1[:, -1] == dup[0]], l2, calib.scan(1), calib.scan(2))[0]
    c1, r1, _ = R.box_param(l1[l1[:, -1] == dup[0]][0], case.calib[1])
    c2, r2, _ = R.box_param(first, case.calib[2])
    np.testing.assert_allclose(rec[15:31].reshape(4, 4), R.box_pose(r2, c2) @ np.linalg.inv(R.box_pose(r1, c1)), rtol=0, atol=1e-12)
    none = np.zeros((0, 9))
    assert P.match_boxes(none, l2, calib.scan(1), calib.scan(2)).shape == (0, 32)
    assert P.match_boxes(l1, np.array([]), calib.scan(1), calib.scan(2)).shape == (0, 32)


def test_match_boxes_record_of_a_turned_box_by_hand():
    """The product's own record for rot = pi / 3 under identity transforms, against numbers worked out by hand (not against the
    restatement, which is written the same way): rotation Rz(-150 deg) row-major, so the length's axis is its first COLUMN
    (-cos 30, -sin 30, 0); half extents l/2 w/2 h/2; T_b1_b2 of a box that keeps its turn and moves by (0.5, -0.25, 0)."""
    c30, s30 = np.sqrt(3) / 2, 0.5
    calib = P.Calibration(np.eye(4), PC.SIMPLE_P, np.eye(4))
    l1 = np.array([[1.0, 2.0, 4.0, 1.0, 2.0, 2.0, np.pi / 3, 0.75, 5.0]])
    l2 = np.array([[1.0, 2.0, 4.0, 1.5, 1.75, 2.0, np.pi / 3, 0.5, 5.0]])
    rec, = P.match_boxes(l1, l2, calib, calib)
    assert rec[0:3].tolist() == [1, 2, 2] and rec[12:15].tolist() == [2, 1, 0.5] and rec[31] == 0.75
    np.testing.assert_allclose(rec[3:12].reshape(3, 3), [[-c30, s30, 0], [-s30, -c30, 0], [0, 0, 1]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(rec[15:31].reshape(4, 4), [[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 0], [0, 0, 0, 1]], rtol=0, atol=1e-15)


def test_calibration_derives_t_radar_camera_and_checks_its_arguments():
    c = P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION, np.eye(4))
    assert np.array_equal(c.t_radar_camera, np.linalg.inv(PC.T_CAMERA_RADAR)) and c.image_size == (1936, 1216) and c.height == (-3.0, 3.0)
    for bad in (lambda: P.Calibration(PC.T_CAMERA_RADAR.astype(np.float32), PC.PROJECTION, np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR[:3], PC.PROJECTION, np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION[:, :3], np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, np.concatenate([PC.PROJECTION, [[0, 0, 0, 1.0]]]), np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION, np.eye(3)),
                lambda: P.Calibration(np.zeros((4, 4)), PC.PROJECTION, np.eye(4)),
                lambda: P.Calibration(np.stack([PC.T_CAMERA_RADAR] * 2), PC.PROJECTION, np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION * np.nan, np.eye(4)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION, np.eye(4), image_size=(0, 10)),
                lambda: P.Calibration(PC.T_CAMERA_RADAR, PC.PROJECTION, np.eye(4), height=(1.0, -1.0))):
        with pytest.raises(ValueError):
            bad()


@pytest.fixture(scope="module")
def good():
    case = PC.chain(3, [40, 50, 60], "pseudo", K=2)
    return case, dict(scans=case.packed_scans, scan_off=case.scan_off, pairs=case.pairs, t_odom_camera=case.odom,
                      tracks=case.packed_tracks, track_off=case.track_off)


def test_every_argument_error_is_a_value_error_before_anything_is_launched(good):
    case, kw = good
    calib = product_calib(case)
    for mode in ("train", "", None, 0):
        with pytest.raises(ValueError):
            P.SplitBuilder(calib, mode, "cpu")
    with pytest.raises(ValueError):
        P.SplitBuilder("calib", "gt", "cpu")
    img = np.zeros((1216, 1936, 2), np.float32)
    bad = {
        "float64 scans": dict(scans=kw["scans"].astype(np.float64)),
        "four columns": dict(scans=kw["scans"][:, :4]),
        "one-dimensional scans": dict(scans=kw["scans"].reshape(-1)),
        "offsets that decrease": dict(scan_off=np.array([0, 90, 40, 150])),
        "offsets that do not start at 0": dict(scan_off=np.array([1, 40, 90, 150])),
        "offsets that do not end at the row count": dict(scan_off=np.array([0, 40, 90, 149])),
        "float offsets": dict(scan_off=case.scan_off.astype(np.float64)),
        "a pair index out of range": dict(pairs=np.array([[0, 1], [1, 3]])),
        "a negative pair index": dict(pairs=np.array([[0, -1]])),
        "pairs of the wrong shape": dict(pairs=np.array([0, 1, 2])),
        "no pairs": dict(pairs=np.zeros((0, 2), np.int64)),
        "float pairs": dict(pairs=case.pairs.astype(np.float64)),
        "poses of the wrong shape": dict(t_odom_camera=case.odom[:2]),
        "float32 poses": dict(t_odom_camera=case.odom.astype(np.float32)),
        "tracks without offsets": dict(track_off=None),
        "eight track columns": dict(tracks=kw["tracks"][:, :8]),
        "float32 tracks": dict(tracks=kw["tracks"].astype(np.float32)),
        "track offsets of the wrong length": dict(track_off=np.array([0, len(kw["tracks"])])),
        "track offsets that decrease": dict(track_off=np.array([0, 5, 2, len(kw["tracks"])])),
        "one image for two pairs": dict(opt_flow=[img]),
        "an image of the wrong size": dict(opt_flow=[img[:, :100], None]),
        "a float64 image": dict(opt_flow=[img.astype(np.float64), None]),
        "clip tags of the wrong length": dict(clip=np.array([0])),
        "float clip tags": dict(clip=np.array([0.0, 1.0])),
    }
    for what, change in bad.items():
        with pytest.raises(ValueError):
            P.SplitBuilder(calib, "pseudo", "cpu").add(**{**kw, **change})
            pytest.fail(what)
    with pytest.raises(ValueError):                                        # optical flow belongs to the pseudo mode
        P.SplitBuilder(calib, "gt", "cpu").add(**kw, opt_flow=[img, None])
    two = P.Calibration(*(np.stack([m] * 2) for m in (PC.T_CAMERA_RADAR, PC.PROJECTION, np.eye(4))))
    with pytest.raises(ValueError):                                        # two calibration sets, three scans
        P.SplitBuilder(two, "gt", "cpu").add(**kw)
    b = P.SplitBuilder(calib, "gt", "cpu")
    for mp in ((0, 1), (1, 0)):
        with pytest.raises(ValueError):
            b.finish(min_points=mp)
    with pytest.raises(ValueError):
        b.finish()                                                         # nothing was added
    for fn in (P.filter_scans, P.count_scans):
        for change in (dict(scans=kw["scans"][:, :4]), dict(scans=kw["scans"].astype(np.float64)), dict(scan_off=np.array([0, 90, 40, 150])),
                       dict(calib=None)):
            with pytest.raises(ValueError):
                fn(**{**dict(scans=kw["scans"], scan_off=case.scan_off, calib=calib, device="cpu"), **change})
    with pytest.raises(ValueError):
        P.filter_scans(kw["scans"], case.scan_off, calib, "cpu", nmax=0)
    pc, n = torch.zeros(3, 3, 8), torch.ones(3, dtype=torch.int32)
    for pairs in ([[0, 3]], [[-1, 0]], [0, 1], np.zeros((0, 2), np.int64)):
        with pytest.raises(ValueError):
            P.pair_batch(pc, pc, n, np.array(pairs))
    with pytest.raises(ValueError):
        P.pair_batch(pc, pc[:, :2], n, np.array([[0, 1]]))
    with pytest.raises(ValueError):
        P.match_boxes(case.tracks[0], case.tracks[1], calib, two)


def test_no_gpu_no_result(good):
    """Valid arguments on a device that is not a GPU: RuntimeError, as everywhere in the product (no CPU fallback)."""
    case, kw = good
    calib = product_calib(case)
    with pytest.raises(RuntimeError):
        P.SplitBuilder(calib, "pseudo", "cpu").add(**kw)
    with pytest.raises(RuntimeError):
        P.SplitBuilder(calib, "gt", "cpu").add(**kw, clip=np.array([0, 0]))
    with pytest.raises(RuntimeError):
        P.filter_scans(kw["scans"], case.scan_off, calib, "cpu")
    with pytest.raises(RuntimeError):
        P.count_scans(torch.from_numpy(kw["scans"]), case.scan_off, calib, torch.device("cpu"))


def test_pair_batch_pairs_the_clouds():
    pc = torch.arange(3 * 3 * 4, dtype=torch.float32).reshape(3, 3, 4)
    ft, n = -pc, torch.tensor([4, 2, 3], dtype=torch.int32)
    b = P.pair_batch(pc, ft, n, np.array([[0, 1], [1, 2], [2, 0]]))
    assert list(b) == ["pc1", "pc2", "ft1", "ft2", "n1", "n2", "interval"]
    assert torch.equal(b["pc1"], pc) and torch.equal(b["pc2"], pc[[1, 2, 0]]) and torch.equal(b["ft2"], ft[[1, 2, 0]])
    assert b["n1"].tolist() == [4, 2, 3] and b["n2"].tolist() == [2, 3, 4] and b["n1"].dtype == torch.int32
    assert b["interval"].tolist() == [np.float32(0.10)] * 3 and all(t.is_contiguous() for t in b.values())


def test_prepare_hip_is_built_contraction_free():
    """The kernels decide pixels and masks from float64 compares that numpy takes with separately rounded products: the Makefile
    builds prepare.hip with -ffp-contract=off, as it builds neighbor.hip."""
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cmflow_amd", "csrc")
    dry = subprocess.run(["make", "-C", csrc, "-n", "-B", "build/prepare.o"], capture_output=True, text=True, check=True).stdout
    line = [l for l in dry.splitlines() if "prepare.hip" in l]
    assert line and "-ffp-contract=off" in line[0], dry
