"""Depth frame in, device-resident point state out: the step between "the camera delivered a depth frame" and the
(4, 6 + uniform_num_pts) state Agent.select_action takes, on the GPU (include/gaddpg.h section A.2, csrc/observe.hip).

The reference does this once per control step in host numpy -- core/utils.py:454-491 (backproject_camera_target[_realworld]),
:308-314 (se3_transform_pc), env/panda_scene.py:442-450, 698-714, 1178-1206 (_get_observation, update_curr_acc_points,
process_pointcloud), core/test_realworld_ros_final.py:826-895 (the same on 640 x 480 frames) -- building a 3 x H*W float64 pixel
grid per frame and, with use_farthest_point, uploading, sampling, downloading and re-uploading the cloud.  Here:

  backproject_depth / cloud_gather_affine / point_state_pack   thin operators over the three entry points
  compose_camera_affine                                        the reference's linear steps composed into one [M | t] (float64, host)
  PointStateBuilder                                            one environment's accumulated cloud and its per-frame state

What the device path costs per frame against the host path was measured by tools/bench_point_state.py
(profiles/point_state.txt, MI355X, both paths ending with the state on the device): 0.71 ms against 2.48 ms at 112 x 112 with
random regularisation, 12.7 ms against 28.9 ms at 640 x 480 with the real-world loop's FPS trims.  Nothing here routes on that
measurement."""
import numpy as np
import torch

from .. import hip
from ..synth_data import HAND_FINGER_POINT

_U16 = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)     # 16 raw bits either way


def _need(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _dense(t, name, dtype, ndim=None):
    """the pointnet2_utils checks: CUDA, contiguous, of the dtype the kernel reads"""
    _need(torch.is_tensor(t) and t.is_cuda, "%s: CPU tensor passed to a libgaddpg operator (CPU not supported)" % name)
    _need(t.is_contiguous(), "%s must be contiguous" % name)
    _need(t.dtype in (dtype if isinstance(dtype, tuple) else (dtype,)), "%s must be a %s tensor" % (name, dtype))
    _need(ndim is None or t.dim() == ndim, "%s must have %s dimensions" % (name, ndim))
    return t


def _cloud(t, name):
    """(B,N,3) or (N,3) float32 CUDA cloud whose points are dense; the clouds may be a strided view into a larger buffer.
    -> (tensor as (B,N,3), stride between clouds in floats)"""
    _need(torch.is_tensor(t) and t.is_cuda, "%s: CPU tensor passed to a libgaddpg operator (CPU not supported)" % name)
    _need(t.dtype == torch.float32, "%s must be a float tensor" % name)
    if t.dim() == 2:
        t = t[None]
    _need(t.dim() == 3 and t.shape[2] == 3, "%s must be (B,N,3) or (N,3)" % name)
    B, N = t.shape[0], t.shape[1]
    if B * N == 0:
        return t, 0
    _need(t.stride(2) == 1 and (N == 1 or t.stride(1) == 3), "%s: the points of a cloud must be contiguous (x, y, z rows of 3 floats)" % name)
    stride = t.stride(0) if B > 1 else 0
    _need(0 <= stride < 2 ** 31, "%s: the stride between clouds must be within [0, 2^31) floats" % name)
    return t, stride


def _affine(A, B, device):
    if A is None:
        return None
    if not torch.is_tensor(A):
        A = torch.as_tensor(np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 12)).to(device)
    A = _dense(A.reshape(-1, 12) if A.is_contiguous() else A, "A", torch.float32, 2)
    _need(A.shape == (B, 12), "A must be (B,12): the rows of [M | t] per cloud")
    return A


def backproject_depth(depth, mask, A, depth_div=None, xyz=None, pix=None, want_pix=True):
    """gad_backproject_depth.  depth (B,H,W) CUDA: float32 metres, or 16-bit integers (torch.uint16, or torch.int16 read as
    unsigned) with depth_div: d = u / depth_div.  mask (B,H,W) uint8 or None.  A (B,12) float32.
    -> xyz (B, H*W, 3) float32 with the kept points of every image compacted to the front in ascending pixel order (rows past
    the count are NOT written: pass `xyz` / `pix` to reuse buffers), count (B,) int32, pix (B, H*W) int32 (None unless want_pix)."""
    _dense(depth, "depth", (torch.float32,) + _U16, 3)
    B, H, W = depth.shape
    u16 = depth.dtype != torch.float32
    _need(not u16 or depth_div is not None, "a 16-bit depth needs depth_div")
    if mask is not None:
        _dense(mask, "mask", torch.uint8, 3)
        _need(mask.shape == depth.shape and mask.device == depth.device, "mask must have the depth's shape and device")
    A = _affine(A, B, depth.device)
    _need(A is not None, "A is required")
    dev = depth.device
    if xyz is None:
        xyz = torch.empty(B, H * W, 3, dtype=torch.float32, device=dev)
    _need(_dense(xyz, "xyz", torch.float32).numel() == B * H * W * 3 and xyz.device == dev, "xyz must be (B, H*W, 3) on the depth's device")
    if pix is None and want_pix:
        pix = torch.empty(B, H * W, dtype=torch.int32, device=dev)
    if pix is not None:
        _need(_dense(pix, "pix", torch.int32).numel() == B * H * W and pix.device == dev, "pix must be (B, H*W) on the depth's device")
    count = torch.empty(B, dtype=torch.int32, device=dev)
    ws = hip.workspace("gad_backproject_depth", dev, B, H, W)
    hip.call("gad_backproject_depth", depth, int(u16), float(depth_div) if u16 else 1.0, mask, A, B, H, W, xyz, count, pix, ws)
    return xyz, count, pix


def _selection(sel, B, device):
    if sel is None:
        return None
    _dense(sel, "sel", torch.int32)
    if sel.dim() == 1:
        sel = sel[None]
    _need(sel.dim() == 2 and sel.shape[0] == B and sel.device == device, "sel must be (B,n) int32 on the cloud's device")
    return sel


def cloud_gather_affine(src, sel=None, A=None, out=None):
    """gad_cloud_gather_affine: out[b][j] = M_b . src[b][sel[b][j]] + t_b.  src (B,N,3) float32 CUDA (or (N,3)), possibly a strided
    view; sel (B,n) int32 or None (identity); A (B,12) or None (copy); out (B,n,3), possibly a view, allocated when None.
    Indices are not range-checked; src and out must not overlap."""
    src, s_stride = _cloud(src, "src")
    B = src.shape[0]
    sel = _selection(sel, B, src.device)
    n = src.shape[1] if sel is None else sel.shape[1]
    A = _affine(A, B, src.device)
    if out is None:
        out = torch.empty(B, n, 3, dtype=torch.float32, device=src.device)
    dst, d_stride = _cloud(out, "out")
    _need(dst.shape[0] == B and dst.shape[1] == n and dst.device == src.device, "out must be (B,n,3) on the cloud's device")
    hip.call("gad_cloud_gather_affine", src, s_stride, sel, A, B, n, dst, d_stride)
    return out


def point_state_pack(src, sel=None, A=None, lead=None, lead_flag=1.0, out=None):
    """gad_point_state_pack: -> state (B, 4, n_lead + n) channel-major; columns [0, n_lead) = lead (n_lead,3) with flag lead_flag,
    column n_lead + j = M_b . src[b][sel[b][j]] + t_b with flag 0.  The inverse of gad_prep_points."""
    src, s_stride = _cloud(src, "src")
    B = src.shape[0]
    sel = _selection(sel, B, src.device)
    n = src.shape[1] if sel is None else sel.shape[1]
    A = _affine(A, B, src.device)
    n_lead = 0
    if lead is not None:
        _dense(lead, "lead", torch.float32, 2)
        _need(lead.shape[1] == 3 and lead.device == src.device, "lead must be (n_lead,3) on the cloud's device")
        n_lead = lead.shape[0]
    if out is None:
        out = torch.empty(B, 4, n_lead + n, dtype=torch.float32, device=src.device)
    _need(_dense(out, "out", torch.float32).numel() == B * 4 * (n_lead + n) and out.device == src.device,
          "out must be (B, 4, n_lead + n) on the cloud's device")
    hip.call("gad_point_state_pack", src, s_stride, sel, A, lead, n_lead, float(lead_flag), B, n, out)
    return out


def compose_camera_affine(K, cam_offset=None, flip_y=True, pose=None, dtype=np.float32):
    """The reference's linear steps from a pixel to a point, composed into the one [M | t] gad_backproject_depth takes; computed
    in float64 on the host, returned as (12,) float32 (rows [M[k][0..2], t_k]; dtype=np.float64 returns it unrounded).

    Derivation.  With p~ = (x, y, 1) and depth d the reference computes, step by step,
        X = d * K^-1 p~                                  core/utils.py:467-470
        X[1] *= -1              i.e. X <- F X            :471, the OpenGL y flip, F = diag(1, -1, 1)   (flip_y; the _realworld variant has none)
        P = C_R X + C_t                                  env/panda_scene.py:446-448, cam_offset = [C_R | C_t]
        P[1] *= -1              i.e. P <- F P            :449, the second y flip (applied with cam_offset, when flip_y)
        Q = R P + T                                      :704, the end-effector pose [R | T]           (pose, optional)
    Every step is linear in X and d is a scalar, so
        Q = d * (R F C_R F K^-1) p~ + (R F C_t + T)  =  d * (M p~) + t.
    The kernel evaluates r = M p~ and d * r + t once, in float32: the chain rounds once per operation of ONE affine instead of
    once per operation of four, and the host does twelve numbers of float64 work per frame instead of 3 x H*W."""
    M = np.linalg.inv(np.asarray(K, dtype=np.float64)[:3, :3])
    t = np.zeros(3)
    F = np.diag([1.0, -1.0, 1.0])
    if flip_y:
        M = F @ M
    if cam_offset is not None:
        C = np.asarray(cam_offset, dtype=np.float64)
        M, t = C[:3, :3] @ M, C[:3, 3].copy()
        if flip_y:
            M, t = F @ M, F @ t
    if pose is not None:
        P = np.asarray(pose, dtype=np.float64)
        M, t = P[:3, :3] @ M, P[:3, :3] @ t + P[:3, 3]
    return np.concatenate((M, t[:, None]), axis=1).reshape(12).astype(dtype)


def pose_affine(pose):
    """rows of pose[:3, :4] as the (12,) float32 affine of the kernels"""
    return np.ascontiguousarray(np.asarray(pose, dtype=np.float64)[:3, :4], dtype=np.float32).reshape(12)


def inverse_pose_affine(pose):
    """the affine of se3_inverse(pose) (reference core/utils.py:446-452: float64 products stored as float32)"""
    P = np.asarray(pose, dtype=np.float64)
    R, T = P[:3, :3], P[:3, 3]
    return np.concatenate((R.T, (-1 * R.T.dot(T))[:, None]), axis=1).astype(np.float32).reshape(12)


class PointStateBuilder(object):
    """One environment's point-cloud state on the device (reference env/panda_scene.py: _get_observation :442-450,
    update_curr_acc_points :698-714, process_pointcloud :1178-1206).

    The accumulated world-frame cloud lives in a device buffer (capacity, 3) that is filled from the back: the reference prepends
    the new points (np.concatenate((new, acc))), here they are written in front of the current start; when the buffer is full it
    doubles (one torch copy).  The random draws are the reference's own np.random.choice calls in the reference's order -- the
    accumulate subsample int(ratio ** env_step * n_new) without replacement, then the regularisation draw -- made on the host
    after reading back the frame's point count (one 4-byte copy) and handed to the kernels as `sel`: a seeded script selects the
    same pixels as the reference.  `rng` (anything with numpy's .choice) replaces the global generator.

    track_provenance=True also keeps, for every accumulated point, (env_step, pixel) of the frame it came from, and sets
    `last_provenance` ((n, 2) int32, the non-lead state columns) in process_pointcloud / observe: bookkeeping for tests and
    debugging, done with torch indexing."""

    def __init__(self, uniform_num_pts=1024, accumulate=True, pt_accumulate_ratio=0.95, regularize=True, use_hand_finger_point=True,
                 hand_flag=1.0, device=None, rng=None, capacity=8192, track_provenance=False, depth_div=5000.0, acc_sample_cap=None):
        self.uniform_num_pts = int(uniform_num_pts)
        self.accumulate = bool(accumulate)
        self.pt_accumulate_ratio = pt_accumulate_ratio
        self.regularize = bool(regularize)
        self.use_hand_finger_point = bool(use_hand_finger_point)
        self.hand_flag = float(hand_flag)
        self.device = torch.device("cuda" if device is None else device)
        self.rng = np.random if rng is None else rng
        self.depth_div = float(depth_div)
        self.track_provenance = bool(track_provenance)
        # None: the simulator's subsample int(ratio ** step * n_new); a number: the real-world loop's
        # min(int(ratio ** step * acc_sample_cap), n_new) (core/test_realworld_ros_final.py:832, cap = uniform_num_pts there)
        self.acc_sample_cap = acc_sample_cap
        # the six gripper key points (data: synth_data.HAND_FINGER_POINT, reference core/utils.py:38-40), point-major
        self.hand_finger_points = torch.as_tensor(np.ascontiguousarray(HAND_FINGER_POINT.T, dtype=np.float32)).to(self.device)
        self._capacity0 = max(int(capacity), 1)
        self._frames = {}          # (H, W, dtype) -> the per-frame buffers of observe
        self.reset()

    # ------------------------------------------------------------------ the accumulated cloud
    def reset(self):
        self._buf = torch.empty(self._capacity0, 3, dtype=torch.float32, device=self.device)
        self._prov = torch.empty(self._capacity0, 2, dtype=torch.int32, device=self.device) if self.track_provenance else None
        self._start = self._capacity0
        self.env_step = 0
        self.last_provenance = None
        self.last_ef_cloud = None
        self.last_fps_idx = None

    @property
    def num_acc_points(self):
        return self._buf.shape[0] - self._start

    @property
    def curr_acc_points(self):
        """the accumulated world-frame cloud, (n, 3) device view, newest points first"""
        return self._buf[self._start:]

    def _reserve(self, k):
        """room for k more points in front of the start (doubling; one torch copy of the live tail)"""
        if k <= self._start:
            return
        n, cap = self.num_acc_points, self._buf.shape[0]
        while cap - n < k:
            cap *= 2
        buf = torch.empty(cap, 3, dtype=torch.float32, device=self.device)
        buf[cap - n:] = self._buf[self._start:]
        if self._prov is not None:
            prov = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
            prov[cap - n:] = self._prov[self._start:]
            self._prov = prov
        self._buf, self._start = buf, cap - n

    def _acc_sample_size(self, n, env_step):
        if self.acc_sample_cap is None:
            return int(self.pt_accumulate_ratio ** env_step * n)
        return min(int(self.pt_accumulate_ratio ** env_step * self.acc_sample_cap), n)

    def _draw(self, n, size, replace):
        # np.random.choice(range(n), ...) of the reference: the integer form draws the same indices from the same stream
        return self.rng.choice(n, size=size, replace=replace)

    def _to_sel(self, index):
        return torch.as_tensor(np.ascontiguousarray(index, dtype=np.int32)).to(self.device, non_blocking=True)[None]

    def _prepend(self, points, index, affine, env_step, pix):
        k = len(index)
        if k == 0:
            return
        self._reserve(k)
        sel = self._to_sel(index)
        cloud_gather_affine(points, sel, affine, out=self._buf[self._start - k:self._start])
        if self._prov is not None:
            src_pix = sel[0] if pix is None else pix[sel[0].long()]
            self._prov[self._start - k:self._start, 0] = int(env_step)
            self._prov[self._start - k:self._start, 1] = src_pix
        self._start -= k

    def update_curr_acc_points(self, new_points, ef_pose, env_step, pix=None):
        """reference :698-714.  new_points (n,3) float32 CUDA in the end-effector frame; ef_pose 4x4 (host).  A subsample of
        int(ratio ** env_step * n) points (acc_sample_cap: see __init__), drawn without replacement, is transformed to the world
        frame and prepended."""
        n = new_points.shape[0]
        index = self._draw(n, self._acc_sample_size(n, env_step), False)
        self._prepend(new_points, index, pose_affine(ef_pose), env_step, pix)

    def regularize_acc(self, npoints, use_farthest_point=False):
        """bring the accumulated cloud to exactly npoints (regularize_pc_point_count on it: the reference's collision_check /
        real-world trimming, core/test_realworld_ros_final.py:842); an empty cloud stays empty"""
        n = self.num_acc_points
        if n == 0 or n == npoints:
            return
        acc = self.curr_acc_points
        if n > npoints and use_farthest_point:
            from ..pointnet2_ops.pointnet2_utils import furthest_point_sample
            sel = furthest_point_sample(acc[None], npoints)
        elif n > npoints:
            sel = self._to_sel(self._draw(n, npoints, False))
        else:
            sel = self._to_sel(np.concatenate((np.arange(n), self._draw(n, npoints - n, True))))
        cap = self._buf.shape[0]
        while cap < npoints:
            cap *= 2
        buf = torch.empty(cap, 3, dtype=torch.float32, device=self.device)
        cloud_gather_affine(acc, sel, None, out=buf[cap - npoints:])
        if self._prov is not None:
            prov = torch.empty(cap, 2, dtype=torch.int32, device=self.device)
            prov[cap - npoints:] = self._prov[self._start:][sel[0].long()]
            self._prov = prov
        self._buf, self._start = buf, cap - npoints

    # ------------------------------------------------------------------ the state
    def process_pointcloud(self, point_state, ef_pose, acc_pt=True, use_farthest_point=False, env_step=None, pix=None):
        """reference :1178-1206.  point_state (n,3) float32 CUDA, this frame's points in the end-effector frame.
        -> (4, n_lead + n_out) float32 CUDA state (3 rows without the hand points)."""
        env_step = self.env_step if env_step is None else env_step
        if self.accumulate and acc_pt:
            self.update_curr_acc_points(point_state, ef_pose, env_step, pix)
            return self._state(self.curr_acc_points, inverse_pose_affine(ef_pose), use_farthest_point,
                               None if self._prov is None else self._prov[self._start:])
        prov = None
        if self.track_provenance:
            src_pix = torch.arange(point_state.shape[0], dtype=torch.int32, device=self.device) if pix is None else pix[:point_state.shape[0]]
            prov = torch.stack((torch.full_like(src_pix, int(env_step)), src_pix), dim=1)
        return self._state(point_state, None, use_farthest_point, prov)

    def _state(self, cloud, affine, use_farthest_point, prov):
        """regularise `cloud` (n,3) under `affine`, prepend the hand points, pack"""
        n, N = cloud.shape[0], self.uniform_num_pts
        sel = None
        self.last_ef_cloud = self.last_fps_idx = None
        if self.regularize and n > 0 and n != N:                 # (an empty cloud skips regularisation: reference :1190)
            if n > N and use_farthest_point:
                from ..pointnet2_ops.pointnet2_utils import furthest_point_sample
                cloud = cloud_gather_affine(cloud, None, affine)[0]      # the end-effector-frame cloud the sampler walks
                affine = None
                sel = furthest_point_sample(cloud[None], N)
                self.last_ef_cloud, self.last_fps_idx = cloud, sel[0]
            elif n > N:
                sel = self._to_sel(self._draw(n, N, False))
            else:
                sel = self._to_sel(np.concatenate((np.arange(n), self._draw(n, N - n, True))))
        lead = self.hand_finger_points if self.use_hand_finger_point else None
        state = point_state_pack(cloud, sel, affine, lead, self.hand_flag)[0]
        if prov is not None:
            self.last_provenance = prov if sel is None else prov[sel[0].long()]
        return state if self.use_hand_finger_point else state[:3]

    def _frame_buffers(self, B, H, W):
        key = (H, W)
        if key not in self._frames:
            self._frames[key] = (torch.empty(B, H * W, 3, dtype=torch.float32, device=self.device),
                                 torch.empty(B, H * W, dtype=torch.int32, device=self.device) if self.track_provenance else None)
        return self._frames[key]

    def _upload(self, a, dtype):
        """a frame (numpy or tensor) on the device; a uint16 array travels as its 16 raw bits, the kernel reads them unsigned"""
        if torch.is_tensor(a):
            return a.to(self.device)
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint16 and dtype is np.float32:
            a = a.view(np.int16)
        elif a.dtype != dtype:
            a = (a != 0).astype(np.uint8) if dtype is np.uint8 else a.astype(dtype)
        return torch.from_numpy(a).to(self.device, non_blocking=True)

    def observe(self, depth, mask, K, ef_pose, env_step, cam_offset=None, flip_y=True, acc=True, use_farthest_point=False):
        """_get_observation :442-450 + process_pointcloud: depth (H,W) float32 metres or uint16 (divided by depth_div), mask (H,W)
        (non-zero = not the target; None = nothing masked), numpy or CUDA tensors; K 3x3, ef_pose 4x4, cam_offset 4x4 (host).
        -> (4, n_lead + uniform_num_pts) float32 CUDA tensor, consumed by Agent.select_action without a host copy.
        With accumulation the frame is back-projected straight into the world frame (the pose is part of the composed affine)
        and the subsample is copied in front of the accumulated cloud; without it, into the end-effector frame."""
        self.env_step = env_step
        depth = self._upload(depth, np.float32)
        if depth.dtype == torch.float64:
            depth = depth.float()
        mask = None if mask is None else self._upload(mask, np.uint8)
        if mask is not None and mask.dtype != torch.uint8:
            mask = (mask != 0).to(torch.uint8)
        H, W = depth.shape[-2], depth.shape[-1]
        accumulate = self.accumulate and acc
        A = compose_camera_affine(K, cam_offset, flip_y, ef_pose if accumulate else None)
        xyz, pix = self._frame_buffers(1, H, W)
        _, count, _ = backproject_depth(depth.reshape(1, H, W), None if mask is None else mask.reshape(1, H, W).contiguous(), A[None],
                                        self.depth_div, xyz=xyz, pix=pix, want_pix=False)
        n = int(count.item())                    # the one read-back of the frame: the draws below need it
        points = xyz[0, :n]
        if accumulate:
            index = self._draw(n, self._acc_sample_size(n, env_step), False)
            self._prepend(points, index, None, env_step, None if pix is None else pix[0])
            return self._state(self.curr_acc_points, inverse_pose_affine(ef_pose), use_farthest_point,
                               None if self._prov is None else self._prov[self._start:])
        return self.process_pointcloud(points, ef_pose, False, use_farthest_point, env_step, None if pix is None else pix[0])
