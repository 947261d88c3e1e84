"""What the native frame loop accepts once the caller lets it track with the RGB-D tracker as well
(native_refusal(..., tracking=True, tracking_rgbd=True), Reconstruction.run_native(tracking=True, tracking_rgbd=True)):
the RGB-D configuration, and nothing else that it refused before.  Needs no device."""
import pytest

from test_native_tracking_host import ICP, PARAMS


def test_both_keywords_admit_the_rgbd_configuration():
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    assert R.native_refusal(icp, use_rgbd_tracking=True, tracking=True, tracking_rgbd=True) is None
    assert R.native_refusal(icp, R.read_render_state(b""), False, True, tracking=True, tracking_rgbd=True) is None
    # the keyword only permits: the plain configuration and recorded poses stay what they were
    assert R.native_refusal(icp, tracking=True, tracking_rgbd=True) is None
    assert R.native_refusal(R.read_app_state(PARAMS), tracking=True, tracking_rgbd=True) is None
    assert R.native_refusal(R.read_app_state(PARAMS), use_rgbd_tracking=True, tracking=True, tracking_rgbd=True) is None


def test_one_keyword_alone_still_refuses_the_rgbd_tracker():
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    assert "RGB-D" in R.native_refusal(icp, use_rgbd_tracking=True, tracking=True)
    assert "RGB-D" in R.native_refusal(icp, use_rgbd_tracking=True, tracking=True, tracking_rgbd=False)
    assert "ICP" in R.native_refusal(icp, use_rgbd_tracking=True)
    # tracking_rgbd means nothing without tracking
    assert "ICP" in R.native_refusal(icp, use_rgbd_tracking=True, tracking_rgbd=True)
    assert "ICP" in R.native_refusal(icp, tracking_rgbd=True)
    assert "ICP" in R.native_refusal(R.read_app_state(PARAMS), use_rgbd_tracking=True, tracking_rgbd=True)


@pytest.mark.parametrize("rgbd", [False, True])
def test_the_new_keyword_keeps_every_other_refusal(rgbd):
    from voxelhashing_amd import reconstruction as R
    icp = R.read_app_state(ICP)
    kw = dict(use_rgbd_tracking=rgbd, tracking=True, tracking_rgbd=True)
    init = R.read_app_state(PARAMS.replace(b"OnlyInit = false", b"OnlyInit = true"))
    assert "s_binaryDumpSensorUseTrajectoryOnlyInit" in R.native_refusal(init, **kw)
    off = R.read_app_state(ICP.replace(b"s_trackingEnabled = true", b"s_trackingEnabled = false"))
    assert "s_trackingEnabled" in R.native_refusal(off, **kw)
    rec = R.read_app_state(ICP + b"s_recordData = true;\n")
    assert "s_recordData" in R.native_refusal(rec, **kw)
    rs = R.read_render_state(b"s_renderToFile = true;\n")
    assert "s_renderToFile" in R.native_refusal(icp, rs, **kw)
    assert "s_bUseCameraCalibration" in R.native_refusal(icp, None, True, **kw)
    # and each of them reads as it does without the keyword
    for state, render, calib in ((init, None, False), (off, None, False), (rec, None, False), (icp, rs, False), (icp, None, True)):
        assert R.native_refusal(state, render, calib, tracking=True, tracking_rgbd=True) == R.native_refusal(state, render, calib, tracking=True)


def test_rgbd_tracking_interface_is_declared():
    """the C ABI names of the feature; bad arguments are refused before anything touches a device"""
    from voxelhashing_amd import engine as E, lib
    for name in ("vh_icp_rgbd_step", "vh_reconstruction_set_tracking_rgbd"):
        assert name in lib.PROTOTYPES, name
    L = lib.load()
    assert L.vh_icp_rgbd_step(0, 0, None, None, None, None, None, None, None, None, None, None, 0.0, 0.0, 0.0, None, 0, None) == 4
    assert L.vh_reconstruction_set_tracking_rgbd(None, None) == 4
    assert callable(E.Reconstruction.setTrackingRGBD)
