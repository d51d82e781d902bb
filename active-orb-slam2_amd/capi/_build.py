"""What the argument builders of the wrapper modules share."""
import numpy as np

_LBA_ARRAYS = (("pose_Tcw", np.float32), ("pose_fixed", np.uint8), ("pose_id", np.int64), ("point_xyz", np.float32),
               ("point_id", np.int64), ("edge_pose", np.int32), ("edge_point", np.int32), ("edge_obs", np.float32),
               ("edge_stereo", np.uint8), ("edge_inv_sigma2", np.float32))


def _batch(Problem, Result, n):
    """the problem and the result array of a call on n items (one element when n is 0), and the empty lists `keep` and `outs`"""
    return (Problem * max(1, n))(), (Result * max(1, n))(), [], []


def _out(shape, dtype, sentinel, default=0, bytewise=False):
    """an output array preset to `default` or, when the caller gave one, to `sentinel`: as the value of every element, or bytewise as
    the value of every byte"""
    if sentinel is None or not bytewise:
        return np.full(shape, default if sentinel is None else sentinel, dtype)
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = sentinel
    return a


def _set_K(s, K, tag=""):
    """K = (fx, fy, cx, cy) -> the float fields fx<tag> .. cy<tag> of the struct s"""
    for name, v in zip(("fx", "fy", "cx", "cy"), K):
        setattr(s, name + tag, float(np.float32(v)))


def _fill_lba_problem(s, prob, keep, missing_is_null=False):
    """the counts and the ten arrays of an aos2_lba_problem_t from a synth_lba_problem()-style dict; `keep` holds the arrays.
    missing_is_null: an array that is absent or None stays NULL (what the argument checks are tried with)"""
    s.n_poses, s.n_points, s.n_edges = prob["n_poses"], prob["n_points"], prob["n_edges"]
    for name, dt in _LBA_ARRAYS:
        if missing_is_null and prob.get(name) is None:
            continue
        a = np.ascontiguousarray(prob[name], dt)
        keep.append(a)
        setattr(s, name, a.ctypes.data)


def _lba_camera_and_stop(s, prob, stop_flag, keep):
    """fx .. bf and the stop flag (a numpy array or None) of an aos2_lba_problem_t"""
    s.fx, s.fy, s.cx, s.cy, s.bf = (float(np.float32(prob[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
    if stop_flag is not None:
        keep.append(stop_flag)
        s.stop_flag = stop_flag.ctypes.data
