"""Named cameras and parameter sets for the tests that hold the camera-model kernels under something other than the
default camera (fx == fy, principal point at the image centre, depth range 0.5-5 m; tests/test_camera_models.py on the
CPU, tests/test_gpu_camera_models.py on the device).  numpy only.

The cameras are given at 640x480 and scaled to a test's size: fx and mx by W / 640, fy and my by H / 480, the
principal point about the pixel centres (so the centre of 640x480 becomes the centre of W x H).  The parameter builders'
defaults stay as they are; everything here goes through their keyword arguments.
"""
import numpy as np

from voxelhashing_amd import synth, vhtypes as T

# name -> fx, fy, mx, my at 640x480
CAMERAS = {
    "tum": (517.3, 516.5, 318.6, 255.3),                 # TUM fr1: a real sensor, fx and fy differ in the fourth digit
    "tall": (525.0, 1.35 * 525.0, 319.5, 239.5),         # block boxes pass 29 rows before 32 columns
    "wide": (1.35 * 525.0, 525.0, 319.5, 239.5),         # the opposite case
    "offcentre": (525.0, 0.93 * 525.0, 319.5 - 0.18 * 640, 239.5 + 0.21 * 480),  # asymmetric frustum, both signs
    "crop": (525.0, 0.93 * 525.0, 1.15 * 640, 239.5),    # a crop of a larger image: every ray leans towards -x
    "fisheyeish": (0.45 * 640, 0.5 * 640, 319.5 + 4.3, 239.5 - 3.1),  # steep rays at the border, long interval lists
}

# name -> keyword arguments of make_depth_camera_params / make_hash_params (voxel = the voxel size), metres the camera
# is moved back along its own axis
PARAMETER_SETS = {
    # S1's front lies 1.5 m and its rim 2.1 m deep from the 2.5 m orbit: every other frame is taken from 0.4 m further
    # back, where the rim lies 2.4 m deep -- beyond the integration distance when it is integrated, and, where a nearer
    # frame has fused it, beyond depth_max when it is ray-cast
    "near": dict(camera=dict(depth_min=0.3, depth_max=2.2), hash=lambda voxel: dict(max_integration_distance=1.9), back=(0.0, 0.4)),
    "thin": dict(camera={}, hash=lambda voxel: dict(truncation=3.2 * voxel, trunc_scale=0.0), back=0.0),
    "thin_scaled": dict(camera={}, hash=lambda voxel: dict(truncation=3.2 * voxel, trunc_scale=4.0 * voxel), back=0.0),
    "saturating": dict(camera={}, hash=lambda voxel: dict(weight_sample=5, weight_max=12), back=0.0),
}

# wider bands than the default one (5 voxels + 2.5 per metre), apart from PARAMETER_SETS, whose keys parametrize tests
# with literal bounds of their own.  thick: 9.6 voxels + 4 per metre -- wider than a block's edge from the first metre on,
# so alloc's ray walk, the interval splat and the fused pass meet other block counts per pixel
BAND_SETS = {
    "thick": dict(camera={}, hash=lambda voxel: dict(truncation=9.6 * voxel, trunc_scale=4.0 * voxel), back=0.0),
}

# name -> (ray increment / truncation, sample-distance threshold / increment, distance threshold / increment): the ray
# caster's step and the two gates a zero crossing passes before it counts, fabsf(lastSdf - dist) < m_thresSampleDist and
# fabsf(dist) < m_thresDist.  The builders' defaults (0.8, 50.5, 50.0) put both thresholds at forty truncations, where
# neither comparison can be false.
MARCH_SETS = {
    "sample_gate": (0.8, 1.0, 50.0),        # rejects by abs(lastSdf - dist) alone
    "dist_gate": (0.8, 50.5, 0.5),          # rejects by abs(dist) alone
    "both_gates": (0.8, 0.9, 0.45),         # both rejections at once
    "fine": (0.25, 50.5, 0.5),              # about four samples in the band, several per block
    "fine_sample_gate": (0.25, 0.9, 50.0),  # the sample gate at the fine step
    "coarse": (2.5, 50.5, 50.0),            # the step is longer than the band
    "coarse_dist_gate": (2.5, 50.5, 0.3),   # the distance gate at the coarse step
}

# the reference's hash sends (x, y, z) and (-x, -y, z) to one bucket; away from the origin an online alloc pass is
# deterministic (tests/test_gpu_frame_loop.py)
OFFSET = np.array([7.3, 5.1, 3.7])
SPHERES = synth.S1_SPHERES.copy()
SPHERES[:, :3] += OFFSET


def intrinsics(name, width, height):
    """fx, fy, mx, my of a named camera at width x height"""
    fx, fy, mx, my = CAMERAS[name]
    sx, sy = width / 640.0, height / 480.0
    return dict(fx=fx * sx, fy=fy * sy, mx=(mx + 0.5) * sx - 0.5, my=(my + 0.5) * sy - 0.5)


def camera(name, width, height, **limits):
    """DepthCameraParams of a named camera (None: the builder's default one)"""
    if name is None:
        return T.make_depth_camera_params(width, height, **limits)
    return T.make_depth_camera_params(width, height, **limits, **intrinsics(name, width, height))


def parameter_set(pset):
    """a set of PARAMETER_SETS or BAND_SETS by its name"""
    return PARAMETER_SETS[pset] if pset in PARAMETER_SETS else BAND_SETS[pset]


def march_factors(march):
    """keyword arguments of make_raycast_params for a set of MARCH_SETS (None: the builder's defaults)"""
    if march is None:
        return {}
    inc, sample, dist = MARCH_SETS[march]
    return dict(ray_increment_factor=inc, thres_sample_dist_factor=sample, thres_dist_factor=dist)


def config(name, size, voxels="P4", pset=None, buckets=1 << 14, blocks=1 << 13, gradients=False, march=None):
    """-> (HashParams, DepthCameraParams, RayCastParams) of a named camera, with a named parameter set (PARAMETER_SETS or
    BAND_SETS) and a named march set (MARCH_SETS) on top"""
    ps = dict(synth.PARAM_SETS[voxels])
    limits = {}
    if pset is not None:
        ps.update(parameter_set(pset)["hash"](ps["voxel_size"]))
        limits = parameter_set(pset)["camera"]
    hp = T.make_hash_params(buckets, blocks, **ps)
    cp = camera(name, *size, **limits)
    return hp, cp, T.make_raycast_params(hp, cp, use_gradients=gradients, **march_factors(march))


def aim(cp):
    """4x4 rotation A: pose @ A turns a camera so that the ray through its image centre points where its optical axis
    pointed (the identity for a centred principal point): what the default camera saw in the middle of its image stays
    in the middle"""
    c = np.array([((cp.m_imageWidth - 1) / 2.0 - cp.mx) / cp.fx, ((cp.m_imageHeight - 1) / 2.0 - cp.my) / cp.fy, 1.0])
    c /= np.linalg.norm(c)
    z = np.array([0.0, 0.0, 1.0])
    v, cosa = np.cross(z, c), float(np.dot(z, c))
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    A = np.eye(4)
    A[:3, :3] = np.eye(3) + K + K @ K / (1.0 + cosa)   # rotates z onto c; as a camera-to-camera map it brings c to z
    A[:3, :3] = A[:3, :3].T
    return A


def place(base_poses, cp, back=0.0, offset=OFFSET):
    """camera-to-world poses (float32[16]) for a named camera from poses made for the default one: moved `back` metres
    along the optical axis (a sequence: taken in turns), aimed (aim), and shifted by `offset` with the scene"""
    A = aim(cp)
    backs = np.atleast_1d(np.asarray(back, np.float64))
    out = []
    for k, p in enumerate(base_poses):
        B = np.eye(4)
        B[2, 3] = -backs[k % len(backs)]
        m = np.asarray(p, np.float64).reshape(4, 4) @ B @ A
        m[:3, 3] += offset
        out.append(m.astype(np.float32).reshape(16))
    return out

