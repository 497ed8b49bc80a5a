"""A float64 numpy restatement of the reference's preprocess step for one frame pair -- the yardstick of tests/test_gpu_prepare.py,
pinned on hand-computed cases by tests/test_prepare_ref.py.  From reading preprocess/utils/get_flow_samples.py:44-175 (get_one_sample),
:178-248 (extract_fg_labels, get_rigid_flow, get_inbox_flow, get_bbx_transformation), :285-312 (get_bbx_param,
filt_points_by_height), optical_flow.py:58-89 (info_from_opt_flow, filt_points_in_fov), vod/frame/transformations.py:285-328
(homogeneous_transformation, project_3d_to_2d), global_param.py:6-7 and, for the loader's side, dataset/vod.py:54-124.

Arrays in, arrays out: no files, no open3d (its oriented box is restated as the closed box |(p - c) . axis| <= extent / 2, its
``transform`` as a 4 x 4 product), nothing from cmflow_amd.  Every decision also reports its MARGIN -- the distance of the compared
quantity from its threshold -- so that a test can require its inputs to sit away from every tie before it compares anything.
"""
import numpy as np

IMG_WIDTH, IMG_HEIGHT = 1936, 1216
HEIGHT = (-3, 3)
INTERVAL = 0.10


class Calib:
    """One frame's transforms: t_camera_radar (4,4), camera_projection_matrix (3,4), t_radar_lidar (4,4), float64."""

    def __init__(self, t_camera_radar, camera_projection_matrix, t_radar_lidar):
        self.t_camera_radar = np.asarray(t_camera_radar, dtype=np.float64)
        self.camera_projection_matrix = np.asarray(camera_projection_matrix, dtype=np.float64)
        self.t_radar_lidar = np.asarray(t_radar_lidar, dtype=np.float64)
        self.t_radar_camera = np.linalg.inv(self.t_camera_radar)


def homogeneous(xyz):
    """(n,3) -> (n,4) float64 with a last column of ones"""
    xyz = np.asarray(xyz, dtype=np.float64)
    return np.hstack([xyz, np.ones((xyz.shape[0], 1))])


def transformed(T, xyz):
    """The points under the 4 x 4 transform T -> (n,3)"""
    return (T @ homogeneous(xyz).T).T[:, :3]


def project(xyz, calib):
    """homogeneous_transformation + project_3d_to_2d -> (uv (n,2) float64 BEFORE rounding, w (n,))"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):     # NaN / Inf rows are the filter's to drop
        uvw = calib.camera_projection_matrix @ (calib.t_camera_radar @ homogeneous(xyz).T)
        uv = uvw[:2] / uvw[2]
    return uv.T, uvw[2]


def filter_scan(scan, calib, image_size=(IMG_WIDTH, IMG_HEIGHT), height=HEIGHT):
    """FOV filter, then height filter -> (source indices of the kept rows in scan order, their (u, v) int64 (n,2), margins).
    A zero or non-finite w is undefined in the reference (astype(int) of NaN); such a row is dropped."""
    scan = np.asarray(scan)
    assert scan.dtype == np.float32 and scan.shape[1] >= 5
    uv, w = project(scan[:, 0:3], calib)
    defined = np.isfinite(w) & (w != 0)
    uvs = np.zeros(uv.shape, dtype=np.int64)
    uvs[defined] = np.round(uv[defined]).astype(np.int64)                  # np.round: half to even
    in_fov = defined & (uvs[:, 0] > 0) & (uvs[:, 0] <= image_size[0]) & (uvs[:, 1] > 0) & (uvs[:, 1] <= image_size[1])
    z = scan[:, 2]                                                         # float32 against the integer bounds
    keep = in_fov & (z >= height[0]) & (z <= height[1])
    idx = np.argwhere(keep).flatten()
    frac = uv[defined] - np.floor(uv[defined])
    margins = {"half_pixel": np.abs(frac - 0.5).reshape(-1)}               # a rounding tie sits at 0
    return idx, uvs[idx], margins


def ego_motion(pose_cam_1, pose_cam_2, calib1, calib2):
    """radar1_radar2, what the sample stores as "trans": frame 2's radar pose expressed in frame 1's radar"""
    radar_pose = [pose @ c.t_camera_radar for pose, c in ((pose_cam_1, calib1), (pose_cam_2, calib2))]
    return np.linalg.inv(radar_pose[0]) @ radar_pose[1]


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def box_param(obj, calib):
    """get_bbx_param for the radar -> (centre (3,), rotation (3,3), extent (l, w, h))"""
    centre = (calib.t_radar_camera @ np.array([obj[3], obj[4], obj[5], 1.0]))[:3]
    rot = calib.t_radar_lidar[:3, :3] @ rot_z(-(obj[6] + np.pi / 2))
    return centre, rot, np.array([obj[2], obj[1], obj[0]])


def box_pose(rot, centre):
    T = np.zeros((4, 4))
    T[:3, :3], T[:3, 3], T[3, 3] = rot, centre, 1.0
    return T


def in_box(xyz, centre, rot, extent):
    """The closed oriented box -> (bool (n,), face margins (n,3): |(p - c) . axis| - extent / 2)"""
    d = (np.asarray(xyz, dtype=np.float64) - centre) @ rot
    face = np.abs(d) - extent / 2
    return (face <= 0).all(axis=1), face


def matched_boxes(labels1, labels2, calib1, calib2):
    """The (box 1, box 2, score) of every frame-1 row that has a frame-2 row of the same id (the FIRST such row), in frame-1 order."""
    labels1, labels2 = np.asarray(labels1, dtype=np.float64), np.asarray(labels2, dtype=np.float64)
    out = []
    if labels1.ndim == 2 and labels2.ndim == 2 and labels1.shape[0] and labels2.shape[0]:
        for obj1 in labels1:
            nxt = np.where(labels2[:, -1] == obj1[-1])[0]
            if len(nxt) != 0:
                out.append((box_param(obj1, calib1), box_param(labels2[nxt[0]], calib2), obj1[-2]))
    return out


def extract_fg(labels1, labels2, xyz1, calib1, calib2):
    """extract_fg_labels -> (fg bool (n,), fg_confs float32 (n,), fg_labels float32 (n,3), margins)"""
    n = len(xyz1)
    fg = np.zeros(n, dtype=bool)
    confs, labels = np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    faces, gates = [], []
    xyz = np.asarray(xyz1, dtype=np.float64)
    for (c1, r1, ext), (c2, r2, _), score in matched_boxes(labels1, labels2, calib1, calib2):
        inside, face = in_box(xyz, c1, r1, ext)
        faces.append(face.reshape(-1))
        if inside.any():
            pts = xyz[inside]
            flow = transformed(box_pose(r2, c2) @ np.linalg.inv(box_pose(r1, c1)), pts) - pts
            far = np.linalg.norm(flow, axis=1).max()
            gates.append(far - 3)
            if far < 3:
                labels[inside] = flow
                confs[inside] = score
                fg[inside] = True
    margins = {"box_face": np.concatenate(faces) if faces else np.zeros(0), "gate": np.array(gates)}
    return fg, confs, labels, margins


def rigid_flow(xyz, radar1_radar2):
    """The flow of static points: their place under inv(radar1_radar2) minus where they are"""
    return transformed(np.linalg.inv(radar1_radar2), xyz) - np.asarray(xyz, dtype=np.float64)


def make_sample(scan1, scan2, calib1, calib2, odom_cam_1, odom_cam_2, labels1, labels2, mode, flow_image=None,
                image_size=(IMG_WIDTH, IMG_HEIGHT), height=HEIGHT):
    """One pair -> (sample, item, extra).
    sample: the reference's dict (pc1, pc2 (n,5) float32; trans = radar1_radar2; opt_info; gt_mask, gt_labels, pse_mask, pse_labels).
    item: the 11-tuple the loader makes of it on a whole frame (dataset/vod.py:54-124 without resampling) -- pos_1, pos_2, feature_1,
      feature_2, trans (inverted, float32), labels, mask, interval, radar_u, radar_v, opt_flow; mode 'gt' = the val / test / train_anno
      branch, 'pseudo' = the train branch.
    extra: idx1, idx2 (source rows kept), margins (every decision's distance from its threshold)."""
    assert mode in ("gt", "pseudo")
    scan1, scan2 = np.asarray(scan1), np.asarray(scan2)
    idx1, uv1, m1 = filter_scan(scan1, calib1, image_size, height)
    idx2, _, m2 = filter_scan(scan2, calib2, image_size, height)
    pc1, pc2 = scan1[idx1][:, 0:5], scan2[idx2][:, 0:5]
    n = pc1.shape[0]
    trans = ego_motion(odom_cam_1, odom_cam_2, calib1, calib2)
    fg, confs, fg_labels, mb = extract_fg(labels1, labels2, pc1[:, 0:3], calib1, calib2)
    gt_mask, gt_labels = np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    pse_mask, pse_labels = np.zeros(n, dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
    margins = {"half_pixel": np.concatenate([m1["half_pixel"], m2["half_pixel"]]), **mb, "moving": np.zeros(0)}
    opt_info = {"radar_u": np.zeros(n), "radar_v": np.zeros(n), "opt_flow": np.zeros((n, 2))}
    if mode == "gt":
        flow_r = rigid_flow(pc1[:, 0:3], trans)
        flow_nr = fg_labels.astype(np.float64) - flow_r                    # float32 labels against the float64 rigid flow
        norm = np.linalg.norm(flow_nr, axis=1)
        margins["moving"] = norm[fg] - 0.05
        moving = fg & (norm > 0.05)
        gt_mask[~moving] = 1
        gt_labels[~moving] = flow_r[~moving]
        gt_labels[moving] = fg_labels[moving]
        gt_mask[moving] = 1 - confs[moving]
        labels, mask = gt_labels, gt_mask
    else:
        pse_mask[~fg] = 1
        pse_labels[fg] = fg_labels[fg]
        pse_mask[fg] = 1 - confs[fg]
        labels, mask = pse_labels, pse_mask
        opt_info["radar_u"], opt_info["radar_v"] = uv1[:, 0].copy(), uv1[:, 1].copy()
        if flow_image is not None:
            opt_info["opt_flow"] = np.asarray(flow_image)[uv1[:, 1] - 1, uv1[:, 0] - 1]
    sample = {"pc1": pc1, "pc2": pc2, "trans": trans, "opt_info": opt_info, "gt_mask": gt_mask, "gt_labels": gt_labels,
              "pse_mask": pse_mask, "pse_labels": pse_labels}
    f32 = lambda a: np.asarray(a).astype(np.float32)
    item = (pc1[:, 0:3], pc2[:, 0:3], pc1[:, [4, 3, 3]], pc2[:, [4, 3, 3]], np.linalg.inv(trans).astype(np.float32), f32(labels),
            f32(mask), INTERVAL, f32(opt_info["radar_u"]), f32(opt_info["radar_v"]), f32(opt_info["opt_flow"]))
    return sample, item, {"idx1": idx1, "idx2": idx2, "margins": margins}


def assert_margins(margins, pixel=1e-6, metric=1e-9):
    """The conditions on the inputs: no projected coordinate within ``pixel`` of a half-integer, no box face, 3 m gate or 0.05 m rule
    within ``metric`` of equality."""
    assert (margins["half_pixel"] >= pixel).all(), margins["half_pixel"].min()
    for k in ("box_face", "gate", "moving"):
        assert (np.abs(margins[k]) >= metric).all(), (k, np.abs(margins[k]).min())
