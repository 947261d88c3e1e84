"""What the native frame loop accepts once the caller lets it track the camera itself (native_refusal(..., tracking=True),
Reconstruction.run_native(tracking=True)): the plain-ICP configuration, and nothing else that it refused before.  Needs no
device."""

PARAMS = b"""
s_sensorIdx = 8;
s_adapterWidth = 160;
s_adapterHeight = 120;
s_trackingEnabled = true;
s_integrationEnabled = true;
s_binaryDumpSensorUseTrajectory = true;
s_binaryDumpSensorUseTrajectoryOnlyInit = false;
"""
ICP = PARAMS.replace(b"s_binaryDumpSensorUseTrajectory = true", b"s_binaryDumpSensorUseTrajectory = false")


def test_default_still_refuses_icp_poses():
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    assert "ICP" in R.native_refusal(icp)
    assert "ICP" in R.native_refusal(icp, tracking=False)
    assert "no tracker" in R.native_refusal(icp)


def test_tracking_admits_the_plain_icp_configuration():
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    assert R.native_refusal(icp, tracking=True) is None
    assert R.native_refusal(icp, R.read_render_state(b""), False, False, tracking=True) is None
    # recorded poses stay what they were: tracking=True only permits, it does not switch the trajectory off
    assert R.native_refusal(R.read_app_state(PARAMS), tracking=True) is None


def test_tracking_keeps_every_other_refusal():
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    assert "RGB-D" in R.native_refusal(icp, use_rgbd_tracking=True, tracking=True)
    assert "RGB-D" in R.native_refusal(R.read_app_state(PARAMS), use_rgbd_tracking=True, tracking=True)
    init = R.read_app_state(PARAMS.replace(b"OnlyInit = false", b"OnlyInit = true"))
    assert "s_binaryDumpSensorUseTrajectoryOnlyInit" in R.native_refusal(init, tracking=True)
    off = R.read_app_state(ICP.replace(b"s_trackingEnabled = true", b"s_trackingEnabled = false"))
    assert "s_trackingEnabled" in R.native_refusal(off, tracking=True)
    rec = R.read_app_state(ICP + b"s_recordData = true;\n")
    assert "s_recordData" in R.native_refusal(rec, tracking=True)
    rs = R.read_render_state(b"s_renderToFile = true;\n")
    assert "s_renderToFile" in R.native_refusal(icp, rs, tracking=True)
    assert "s_bUseCameraCalibration" in R.native_refusal(icp, None, True, tracking=True)


def test_tracking_interface_is_declared():
    """the C ABI names of the feature; bad arguments are refused before anything touches a device"""
    from voxelhashing_amd import lib
    for name in ("vh_icp_step", "vh_icp_publish", "vh_reconstruction_set_tracking", "vh_reconstruction_get_poses", "vh_reconstruction_get_tracking_stats"):
        assert name in lib.PROTOTYPES, name
    L = lib.load()
    assert L.vh_icp_step(None, None, None, None, 0, 0, 0.0, 0.0, 0.0, None, None, None, None, 0.0, 0.0, 0.0, None, 0, None) == 4
    assert L.vh_reconstruction_set_tracking(None, None) == 4 and L.vh_reconstruction_get_poses(None, 0, 0, None) == 4
    assert L.vh_reconstruction_get_tracking_stats(None, None, None) == 4
