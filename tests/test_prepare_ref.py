"""CPU: tests/prepare_ref.py (the float64 restatement of the reference's preprocess step) on cases computed by hand."""
import numpy as np

import prepare_ref as R

I4 = np.eye(4)
# a camera looking along the radar's z axis: u = 100 x / z + 968, v = 100 y / z + 608
P = np.array([[100.0, 0, 968, 0], [0, 100.0, 608, 0], [0, 0, 1, 0]])
CAL = R.Calib(I4, P, I4)
AXIS = -np.pi / 2                                    # the rot that aligns a box with t_radar_lidar


def scan(*xyz):
    """rows x y z RCS v_r with RCS = 10 + i, v_r = -i"""
    return np.array([[x, y, z, 10 + i, -i] for i, (x, y, z) in enumerate(xyz)], dtype=np.float32)


def box(x, y, z, id, score=0.75, l=2.0, w=1.0, h=1.0, rot=AXIS):
    return [h, w, l, x, y, z, rot, score, id]


def sample(pts, l1, l2, mode, odom2=I4, **kw):
    s1 = scan(*pts)
    return R.make_sample(s1, s1, CAL, CAL, I4, odom2, np.array(l1, dtype=np.float64), np.array(l2, dtype=np.float64), mode, **kw)


def test_a_point_on_the_optical_axis_lands_on_the_principal_point():
    uv, w = R.project(np.array([[0.0, 0.0, 2.5]]), CAL)
    assert uv.tolist() == [[968.0, 608.0]] and w.tolist() == [2.5]
    idx, uvs, _ = R.filter_scan(scan((0, 0, 2.5), (1, -2, 2)), CAL)
    assert idx.tolist() == [0, 1] and uvs.tolist() == [[968, 608], [1018, 508]]


def test_the_filter_bounds_rounding_and_the_missing_depth_test():
    # u = 968 + 100 x at z = 1: 0 is outside, 1 inside, 1936 inside, 1937 outside; half to even: 968.5 -> 968, 969.5 -> 970
    xs = [(-9.68, 0, 1), (-9.67, 0, 1), (9.68, 0, 1), (9.69, 0, 1), (0.005, 0, 1), (0.015, 0, 1)]
    idx, uvs, _ = R.filter_scan(np.array([[x, y, z, 0, 0] for x, y, z in xs], dtype=np.float64).astype(np.float32), CAL)
    assert idx.tolist() == [1, 2, 4, 5] and uvs[:2, 0].tolist() == [1, 1936]
    up = np.nextafter(np.float32(3), np.float32(4))
    idx, _, _ = R.filter_scan(scan((0, 0, 3), (0, 0, up), (0, 0, -3), (0, 0, -up), (0, 0, 0)), CAL)
    assert idx.tolist() == [0, 2]                                          # z = +-3 kept; z = -3 lies BEHIND this camera: no depth test
    assert R.filter_scan(scan((0, 0, 0)), CAL)[0].size == 0                # w = 0: dropped


def test_rot_minus_half_pi_aligns_the_box_with_t_radar_lidar():
    t_rl = np.eye(4)
    t_rl[:3, :3] = R.rot_z(0.3) @ np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    centre, rot, extent = R.box_param(box(1, 2, 3, 7, l=4, w=2, h=1), R.Calib(I4, P, t_rl))
    assert np.array_equal(rot, t_rl[:3, :3]) and centre.tolist() == [1, 2, 3] and extent.tolist() == [4, 2, 1]
    inside, _ = R.in_box(np.array([[2.9, 2, 3], [3.1, 2, 3], [3.0, 2.0, 3.0], [1, 3.01, 3]]), np.array([1.0, 2, 3]), np.eye(3), extent)
    assert inside.tolist() == [True, False, True, False]                   # the box is closed


def test_identity_poses_give_zero_rigid_flow():
    _, item, _ = sample([(0, 0, 2), (1, 1, 1.5), (-2, 0.5, 2.5)], [], [], "gt")
    assert np.array_equal(item[5], np.zeros((3, 3), np.float32)) and item[6].tolist() == [1, 1, 1]
    assert np.array_equal(item[4], np.eye(4, dtype=np.float32))
    assert not item[8].any() and not item[9].any() and not item[10].any() and item[7] == 0.10
    assert np.array_equal(item[2], np.array([[0, 10, 10], [-1, 11, 11], [-2, 12, 12]], np.float32))       # v_r RCS RCS


def test_ego_motion_gives_the_rigid_flow_of_static_points():
    odom2 = np.eye(4)
    odom2[:3, 3] = [0.5, 0, 0]                                             # the sensor moves +0.5 in x: static points move -0.5
    sam, item, _ = sample([(0, 0, 2), (1, 1, 1.5)], [], [], "gt", odom2=odom2)
    assert np.array_equal(sam["trans"][:3, 3], [0.5, 0, 0]) and np.array_equal(item[4][:3, 3], np.float32([-0.5, 0, 0]))
    assert np.array_equal(item[5], np.float32([[-0.5, 0, 0], [-0.5, 0, 0]]))


def test_a_translated_box_gives_its_translation_as_flow():
    pts = [(0.5, 0, 2), (3, 0, 2), (-0.96, 0.48, 2.4)]                    # the second one is outside the 2 x 1 x 1 box at (0, 0, 2)
    _, item, ex = sample(pts, [box(0, 0, 2, 5)], [box(0.25, -0.5, 2, 5)], "pseudo")
    assert np.array_equal(item[5], np.float32([[0.25, -0.5, 0], [0, 0, 0], [0.25, -0.5, 0]]))
    assert item[6].tolist() == [0.25, 1, 0.25]                             # 1 - score on foreground
    assert item[8].tolist() == [993, 1118, 928] and item[9].tolist() == [608, 608, 628]
    R.assert_margins(ex["margins"])
    assert ex["margins"]["box_face"].size == 9 and np.isclose(ex["margins"]["gate"][0], np.hypot(0.25, 0.5) - 3)


def test_the_flow_image_is_read_at_v_minus_1_u_minus_1():
    img = np.zeros((R.IMG_HEIGHT, R.IMG_WIDTH, 2), np.float32)
    img[607, 992], img[607, 1117] = (1.5, -2.5), (3, 4)
    _, item, _ = sample([(0.5, 0, 2), (3, 0, 2)], [], [], "pseudo", flow_image=img)
    assert item[10].tolist() == [[1.5, -2.5], [3, 4]]
    assert not sample([(0.5, 0, 2)], [], [], "gt", flow_image=img)[1][10].any()


def test_the_three_metre_gate():
    pts = [(0.5, 0, 2)]
    for shift, is_fg in ((2.9, True), (3.5, False)):
        _, item, ex = sample(pts, [box(0, 0, 2, 5)], [box(shift, 0, 2, 5)], "pseudo")
        assert item[6].tolist() == [0.25 if is_fg else 1.0] and item[5][0, 0] == (np.float32(shift) if is_fg else 0)
        assert np.isclose(ex["margins"]["gate"][0], shift - 3)


def test_the_moving_rule_of_five_centimetres():
    for shift, moving in ((0.04, False), (0.06, True)):
        _, item, ex = sample([(0.5, 0, 2)], [box(0, 0, 2, 5)], [box(shift, 0, 2, 5)], "gt")
        assert item[6].tolist() == [0.25 if moving else 1.0]
        assert item[5][0].tolist() == [np.float32(shift) if moving else 0, 0, 0]       # not moving: the rigid flow, here 0
        assert np.isclose(ex["margins"]["moving"][0], shift - 0.05, atol=1e-7)


def test_the_first_row_of_an_id_in_frame_two_is_taken_and_unmatched_rows_are_skipped():
    l2 = [box(9, 9, 9, 4), box(0.5, 0, 2, 5), box(-1, 0, 2, 5)]
    _, item, _ = sample([(0.5, 0, 2)], [box(0, 0, 2, 6), box(0, 0, 2, 5)], l2, "pseudo")
    assert item[5][0].tolist() == [0.5, 0, 0]
    assert len(R.matched_boxes(np.array([box(0, 0, 2, 6)]), np.array(l2), CAL, CAL)) == 0
    assert R.matched_boxes(np.zeros(0), np.array(l2), CAL, CAL) == []      # a frame without rows: nothing is foreground


def test_a_later_box_overwrites_an_earlier_one():
    pts = [(0.5, 0, 2), (-0.5, 0, 2), (1.5, 0, 2)]                         # in both | in the first only | in the second only
    l1 = [box(0, 0, 2, 1, score=0.5), box(1, 0, 2, 2, score=0.25)]
    l2 = [box(0, 1, 2, 1), box(1, 0, 2.5, 2)]
    _, item, _ = sample(pts, l1, l2, "pseudo")
    assert item[5].tolist() == [[0, 0, 0.5], [0, 1, 0], [0, 0, 0.5]] and item[6].tolist() == [0.75, 0.5, 0.75]
    _, item, _ = sample(pts, l1[::-1], l2, "pseudo")
    assert item[5].tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0.5]] and item[6].tolist() == [0.5, 0.5, 0.75]


def test_a_turned_box_has_its_length_along_the_turned_axis():
    """rot = pi / 3: the box's rotation is Rz(-(pi/3 + pi/2)) = Rz(-150 deg), whose first column -- the axis of the LENGTH -- is
    (-cos 30, -sin 30, 0): the 4 x 1 box lies along the direction (cos 30, sin 30).  A point 1.8 m out along that direction is inside;
    its mirror images are 1.56 m off the axis and outside (what a wrong sign of the angle, rows as axes, or a dropped pi / 2 would
    take for inside), and a point 0.4 m across is inside while 0.6 m across is not."""
    c30, s30 = np.sqrt(3) / 2, 0.5
    centre, rot, extent = R.box_param(box(1, 2, 2, 7, l=4, w=1, h=1, rot=np.pi / 3), CAL)
    assert np.allclose(rot, [[-c30, s30, 0], [-s30, -c30, 0], [0, 0, 1]], rtol=0, atol=1e-15) and extent.tolist() == [4, 1, 1]
    along, across = np.array([c30, s30, 0]), np.array([-s30, c30, 0])
    pts = centre + np.array([1.8 * along, 1.8 * along * [1, -1, 1], 1.8 * along * [-1, 1, 1], -1.8 * along, 0.4 * across, 0.6 * across,
                             1.8 * across])
    assert R.in_box(pts, centre, rot, extent)[0].tolist() == [True, False, False, True, True, False, False]
    # the flow of a box that turns about its own centre by 90 degrees: a point 1 m out along the length moves to 1 m across
    l1, l2 = [box(0, 0, 2, 5, l=4, w=1, rot=np.pi / 3)], [box(0, 0, 2, 5, l=4, w=1, rot=np.pi / 3 - np.pi / 2)]
    _, item, _ = sample([(c30, s30, 2)], l1, l2, "pseudo")
    assert np.allclose(item[5][0], [-s30 - c30, c30 - s30, 0], rtol=0, atol=1e-6) and item[6].tolist() == [0.25]
