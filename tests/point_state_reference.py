"""numpy restatements behind the point-state tests (tests/test_point_state_host.py, tests/test_gpu_point_state.py).

Parity pinned by reading, not by import: the reference's env / vision modules need transforms3d, pybullet and others that are not
installed here, so the cited lines are restated -- reference core/utils.py:308-314 (se3_transform_pc), :446-452 (se3_inverse),
:454-491 (backproject_camera_target[_realworld]), :784-813 (regularize_pc_point_count), env/panda_scene.py:442-450
(_get_observation), :698-714 (update_curr_acc_points), :1178-1206 (process_pointcloud).

Two kinds of restatement live here:
  * the REFERENCE CHAIN, step by step as the reference computes it, in a chosen dtype: float64 is the reference itself, float32
    (every array cast, every product a float32 numpy product) is the yardstick of the project's 3x float64-gate rule;
  * the DOCUMENTED ORDER of the kernels (include/gaddpg.h section A.2) in float32 numpy, where every operator rounds once: what
    the device results must equal bit for bit."""
import numpy as np

# the six gripper key points of reference core/utils.py:38-40 (data), (3, 6)
HAND_FINGER_POINT = np.array([[0., 0., 0., -0., 0., -0.],
                              [0., 0., 0.053, -0.053, 0.053, -0.053],
                              [0., 0., 0.075, 0.075, 0.105, 0.105]])


# ---------------------------------------------------------------------------------------------------------------------
# the reference chain
# ---------------------------------------------------------------------------------------------------------------------
def keep_mask(depth, mask):
    """utils.py:459-460: (depth != 0) * (mask == 0) on the flattened float32 depth -- a NaN depth is kept"""
    d = np.asarray(depth).astype(np.float32, copy=True).flatten()
    keep = d != 0
    if mask is not None:
        keep = keep * (np.asarray(mask).flatten() == 0)
    return d, keep


def se3_inverse(RT, dtype=np.float64):
    """utils.py:446-452 (the result is a float32 matrix whatever the input)"""
    RT = np.asarray(RT).astype(dtype)
    R, T = RT[:3, :3], RT[:3, 3].reshape((3, 1))
    out = np.eye(4, dtype=np.float32)
    out[:3, :3] = R.transpose()
    out[:3, 3] = -1 * np.dot(R.transpose(), T).reshape(3)
    return out


def se3_transform(pose, points, dtype=np.float64):
    """utils.py:308-310 on a (3, n) cloud"""
    pose = np.asarray(pose).astype(dtype)
    return (pose[:3, :3].dot(np.asarray(points).astype(dtype)) + pose[:3, [3]]).astype(dtype)


def backproject_chain(depth, K, mask, cam_offset=None, flip_y=True, pose=None, dtype=np.float64):
    """utils.py:454-472 (flip_y=False: :474-491), then panda_scene.py:446-449 when cam_offset is given, then :704 when pose is
    given; every step in `dtype`.  -> ((3, n) points, (n,) source pixels)"""
    Kinv = np.linalg.inv(np.asarray(K, dtype=np.float64)).astype(dtype)
    height, width = depth.shape
    d, keep = keep_mask(depth, mask)
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    ones = np.ones((height, width), dtype=np.float32)
    x2d = np.stack((x, y, ones), axis=2).reshape(width * height, 3).astype(dtype)
    with np.errstate(invalid="ignore"):
        R = Kinv.dot(x2d.transpose())
        X = np.multiply(np.tile(d.reshape(1, width * height), (3, 1)).astype(dtype), R)
        if flip_y:
            X[1] *= -1
        X = X[:, keep]
        if cam_offset is not None:
            X = se3_transform(cam_offset, X, dtype)
            if flip_y:
                X[1] *= -1
        if pose is not None:
            X = se3_transform(pose, X, dtype)
    return X, np.flatnonzero(keep)


def compose_chain64(K, cam_offset=None, flip_y=True, pose=None):
    """the [M | t] of the chain above, found by pushing the origin and the three unit pixels through it in float64 (no algebra
    shared with compose_camera_affine): point(d, p~) = d * M p~ + t"""
    F = np.diag([1.0, -1.0, 1.0])

    def chain(v):                                   # v = d * p~ as a (3, 1) column
        X = np.linalg.inv(np.asarray(K, dtype=np.float64)).dot(v)
        if flip_y:
            X = F.dot(X)
        if cam_offset is not None:
            X = se3_transform(cam_offset, X)
            if flip_y:
                X = F.dot(X)
        if pose is not None:
            X = se3_transform(pose, X)
        return X[:, 0]

    t = chain(np.zeros((3, 1)))
    M = np.stack([chain(np.eye(3)[:, [i]]) - t for i in range(3)], axis=1)
    return np.concatenate((M, t[:, None]), axis=1).reshape(12)


class ReferenceScene(object):
    """_get_observation / update_curr_acc_points / process_pointcloud of env/panda_scene.py restated in `dtype`, with the
    provenance (env_step, pixel) of every point carried along the same index operations.  The np.random.choice calls are the
    reference's, in the reference's order."""

    def __init__(self, uniform_num_pts=1024, accumulate=True, pt_accumulate_ratio=0.95, regularize=True,
                 use_hand_finger_point=True, dtype=np.float64):
        self.uniform_num_pts, self.accumulate, self.ratio = uniform_num_pts, accumulate, pt_accumulate_ratio
        self.regularize, self.use_hand, self.dtype = regularize, use_hand_finger_point, dtype
        self.curr_acc_points = np.zeros([3, 0], dtype=dtype)
        self.acc_prov = np.zeros([2, 0], dtype=np.int64)

    def update_curr_acc_points(self, new_points, prov, ef_pose, env_step):          # :698-714
        new_points = se3_transform(ef_pose, new_points, self.dtype)
        index = np.random.choice(range(new_points.shape[1]), size=int(self.ratio ** env_step * new_points.shape[1]),
                                 replace=False).astype(int)
        self.curr_acc_points = np.concatenate((new_points[:, index], self.curr_acc_points), axis=1)
        self.acc_prov = np.concatenate((prov[:, index], self.acc_prov), axis=1)

    def regularize_pc_point_count(self, pc, prov, npoints):                        # utils.py:784-813, random branches
        if pc.shape[0] > npoints:
            index = np.random.choice(range(pc.shape[0]), size=npoints, replace=False)
            return pc[index, :], prov[:, index]
        if pc.shape[0] < npoints:
            index = np.random.choice(range(pc.shape[0]), size=npoints - pc.shape[0])
            return np.concatenate((pc, pc[index, :]), axis=0), np.concatenate((prov, prov[:, index]), axis=1)
        return pc, prov

    def process_pointcloud(self, point_state, prov, ef_pose, env_step, acc_pt=True):  # :1178-1206
        if self.accumulate and acc_pt:
            self.update_curr_acc_points(point_state, prov, ef_pose, env_step)
            inv = se3_inverse(ef_pose, self.dtype)
            point_state, prov = se3_transform(inv, self.curr_acc_points, self.dtype), self.acc_prov
        if self.regularize and point_state.shape[1] > 0:
            pc, prov = self.regularize_pc_point_count(point_state.T, prov, self.uniform_num_pts)
            point_state = pc.T
        if self.use_hand:
            hand = HAND_FINGER_POINT.astype(self.dtype)
            point_state = np.concatenate([hand, point_state], axis=1)
            point_state_ = np.zeros((4, point_state.shape[1]), dtype=self.dtype)
            point_state_[:3] = point_state
            point_state_[3, :hand.shape[1]] = 1
            point_state = point_state_
        return point_state, prov

    def get_observation(self, depth, mask, K, cam_offset, ef_pose, env_step, acc=True):   # :442-450
        point_state, pix = backproject_chain(depth, K, mask, cam_offset, True, None, self.dtype)
        prov = np.stack((np.full(pix.shape, env_step, dtype=np.int64), pix.astype(np.int64)))
        return self.process_pointcloud(point_state, prov, ef_pose, env_step, acc)


# ---------------------------------------------------------------------------------------------------------------------
# the documented order of the kernels, float32 numpy (every operator below rounds once; numpy never contracts)
# ---------------------------------------------------------------------------------------------------------------------
def documented_depth(depth, div=None):
    """metres as the kernel reads them: float32 as it is, uint16 through one IEEE division"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(np.float32) / np.float32(div)
    return depth.astype(np.float32)


def documented_backproject(depth, mask, A, div=None):
    """gad_backproject_depth on ONE image: -> xyz (n, 3) float32, pix (n,) int32 (n = the count)"""
    h, w = depth.shape
    d, keep = keep_mask(documented_depth(depth, div), mask)
    p = np.flatnonzero(keep)
    x, y, dk = (p % w).astype(np.float32), (p // w).astype(np.float32), d[p]
    A = np.asarray(A, dtype=np.float32).reshape(3, 4)
    out = np.empty((p.size, 3), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            r = (A[k, 0] * x + A[k, 1] * y) + A[k, 2]
            out[:, k] = dk * r + A[k, 3]
    return out, p.astype(np.int32)


def documented_affine(A, pts):
    """((M[k][0] * x + M[k][1] * y) + M[k][2] * z) + t_k on (n, 3) float32 points; A None copies"""
    pts = np.asarray(pts, dtype=np.float32)
    if A is None:
        return pts.copy()
    A = np.asarray(A, dtype=np.float32).reshape(3, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    for k in range(3):
        out[:, k] = ((A[k, 0] * x + A[k, 1] * y) + A[k, 2] * z) + A[k, 3]
    return out


def documented_gather(src, sel, A):
    """gad_cloud_gather_affine: src (B, N, 3), sel (B, n) or None, A (B, 12) or None -> (B, n, 3)"""
    B = src.shape[0]
    return np.stack([documented_affine(None if A is None else A[b], src[b] if sel is None else src[b][sel[b]]) for b in range(B)])


def documented_pack(src, sel, A, lead, lead_flag):
    """gad_point_state_pack -> (B, 4, n_lead + n)"""
    pts = documented_gather(src, sel, A)
    B, n = pts.shape[0], pts.shape[1]
    n_lead = 0 if lead is None else lead.shape[0]
    out = np.zeros((B, 4, n_lead + n), dtype=np.float32)
    if n_lead:
        out[:, :3, :n_lead] = np.asarray(lead, dtype=np.float32).T
        out[:, 3, :n_lead] = np.float32(lead_flag)
    out[:, :3, n_lead:] = pts.transpose(0, 2, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# seeded cases
# ---------------------------------------------------------------------------------------------------------------------
def random_pose(rng, shift=0.3):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    P = np.eye(4)
    P[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    P[:3, 3] = rng.uniform(-shift, shift, size=3)
    return P


def intrinsics(H, W):
    """a pinhole camera whose field of view covers the image (focal length = the larger side)"""
    f = float(max(H, W))
    return np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])


def random_frame(rng, H, W, zero_frac=0.2, mask_frac=0.3):
    """a depth image in metres with holes, and a mask (non-zero = not the target)"""
    depth = rng.uniform(0.3, 1.2, size=(H, W)).astype(np.float32)
    depth[rng.random((H, W)) < zero_frac] = 0.0
    mask = (rng.random((H, W)) < mask_frac).astype(np.uint8) * rng.integers(1, 255, size=(H, W)).astype(np.uint8)
    return depth, mask
