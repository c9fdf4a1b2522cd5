"""CPU: the host description of a rig of cameras that differ (simpb_amd/preprocess.py: CameraSource, RigPlan). The rig's
per-camera tables are the tables a ResamplePlan computes for that camera alone -- not a restatement of them -- and the two
things a caller takes away from a rig, the image transforms and the 2D back-mapping table, equal their closed forms."""
import numpy as np
import pytest

from simpb_amd import _lib
from simpb_amd import preprocess as P

P010_LAYOUT = dict(pitch=192, luma_rows=56)


def sources(width=40):
    """Five cameras to a common `width` x 24 output: every format, an up-scaling and an unresampled axis, a flip."""
    d = 40 - width
    return [P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44 - d, 28))),
            P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41 - d, 25)), "nv12", layout=dict(pitch=176)),
            P.CameraSource((48, 80), dict(resize=0.5, crop=(0, 0, 40 - d, 24), flip=True), "p010", "bt709", P010_LAYOUT),
            P.CameraSource((30, 50), dict(resize=1, crop=(5, 3, 45 - d, 27)), "nv21", layout=dict(pitch=54)),
            P.CameraSource((12, 20), dict(resize=2, crop=(d, 0, 40, 24)))]


def test_tables_are_each_cameras_own_plan():
    rig = P.RigPlan(sources())
    assert rig.out_hw == (24, 40) and rig.num_cams == 5
    for c, s in enumerate(rig.sources):
        alone = P.ResamplePlan(s.src_hw, s.aug_config, None, s.frame_format, s.colour, s.surface)
        for name in ("kx", "xlo", "xn", "ky", "ylo", "yn"):
            a, b = getattr(rig, name)[c], getattr(alone, name)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (c, name)
        for name in ("taps_x", "taps_y", "src_row0", "src_rows", "flip", "yuv"):
            assert getattr(rig, name)[c] == getattr(alone, name), (c, name)
        assert rig.surfaces[c].key == alone.surface.key and rig.surfaces[c].frame_format == alone.frame_format
    assert np.array_equal(rig.lut.view(np.uint16), P.normalise_lut().view(np.uint16))
    # what the Pillow rule gives for these cameras (re-derived, not trusted)
    assert [P.coefficients(w, d)[2].shape[1] for w, d in ((96, 48), (168, 42), (80, 40), (50, 50), (20, 40))] == list(rig.taps_x) == [9, 17, 9, 1, 5]
    assert len(set(rig.src_rows)) > 1


def test_descriptors_and_offsets():
    rig = P.RigPlan(sources())
    cams = rig.descriptors()
    assert len(cams) == 5 and isinstance(cams[0], _lib.RigCamera)
    kx = ky = x = y = rows = 0
    for c, d in enumerate(cams):
        assert (d.kx_offset, d.x_offset, d.ky_offset, d.y_offset, d.mid_row) == (kx, x, ky, y, rows), c
        kx, x, ky, y, rows = kx + 40 * rig.taps_x[c], x + 40, ky + 24 * rig.taps_y[c], y + 24, rows + rig.src_rows[c]
        sf = rig.surfaces[c]
        assert (d.format, d.src_height, d.src_width) == (P.SURFACE_FORMAT[sf.frame_format],) + sf.src_hw
        assert (d.pitch, d.chroma_pitch, d.chroma_offset) == (sf.pitch, sf.chroma_pitch, sf.chroma_offset)
        assert (d.src_row0, d.src_rows, d.taps_x, d.taps_y, d.flip) == (rig.src_row0[c], rig.src_rows[c], rig.taps_x[c], rig.taps_y[c], int(c == 2))
    assert rig.mid_rows == rows == sum(rig.src_rows)
    assert (cams[2].yoff, cams[2].iy) == P.p010_coefficients("bt709")[:2] and cams[0].iy == 1


def test_refusals():
    good = sources()
    with pytest.raises(ValueError, match="camera 4: 38 x 24"):
        P.RigPlan(good[:4] + [P.CameraSource((12, 20), dict(resize=2, crop=(2, 0, 40, 24)))])
    with pytest.raises(ValueError, match="1 .. 16 cameras, got 0"):
        P.RigPlan([])
    with pytest.raises(ValueError, match="1 .. 16 cameras, got 17"):
        P.RigPlan([good[0]] * 17)
    assert P.RigPlan([good[0]] * 16).num_cams == 16 and P.RigPlan(good[:1]).num_cams == 1
    with pytest.raises(ValueError, match="resize_dims"):
        P.CameraSource((64, 96), dict(resize_dims=(48, 32), crop=(4, 4, 44, 28)))
    with pytest.raises(ValueError, match="does not describe"):          # a layout of another size
        P.CameraSource((64, 96), dict(resize=0.5), "nv12", layout=P.SurfaceLayout((48, 80), "nv12"))
    with pytest.raises(ValueError, match="does not describe"):          # ... of another format
        P.CameraSource((64, 96), dict(resize=0.5), "nv12", layout=P.SurfaceLayout((64, 96), "p010"))
    with pytest.raises(ValueError, match="rows overlap"):
        P.CameraSource((64, 96), dict(resize=0.5), "nv12", layout=dict(pitch=95))
    with pytest.raises(ValueError, match="jfif"):
        P.CameraSource((48, 80), dict(resize=0.5), "p010")
    with pytest.raises(ValueError, match="CameraSource"):
        P.RigPlan([good[0], dict(resize=0.5)])


def test_image_transforms_closed_form():
    rig = P.RigPlan(sources())
    m = rig.image_transforms()
    assert m.dtype == np.float64 and m.shape == (5, 3, 3)
    assert np.array_equal(m[0], np.array([[0.5, 0, -4], [0, 0.5, -4], [0, 0, 1]]))
    assert np.array_equal(m[1], np.array([[0.25, 0, -1], [0, 0.25, -1], [0, 0, 1]]))
    assert np.array_equal(m[2], np.array([[-0.5, 0, 40], [0, 0.5, 0], [0, 0, 1]]))          # flip: x -> crop width - x
    assert np.array_equal(m[3], np.array([[1.0, 0, -5], [0, 1, -3], [0, 0, 1]]))
    assert np.array_equal(m[4], np.array([[2.0, 0, 0], [0, 2, 0], [0, 0, 1]]))
    # resize, crop and flip together: a source pixel (u, v) lands at (W - (r u - x0), r v - y0)
    s = P.CameraSource((64, 96), dict(resize=0.5, crop=(4, 4, 44, 28), flip=True))
    got = P.RigPlan([s]).image_transforms()[0] @ np.array([10.0, 20.0, 1.0])
    assert np.array_equal(got, np.array([40 - (0.5 * 10 - 4), 0.5 * 20 - 4, 1.0]))


def test_box2d_table_is_the_scalar_entry_points_arithmetic():
    t = P.RigPlan(sources()).box2d_table()
    assert t.dtype == np.float32 and t.shape == (5, 4)
    one = np.float32(1.0)
    want = [(40, 24, 4, one / np.float32(0.5)), (40, 24, 1, one / np.float32(0.25)), (40, 24, 0, one / np.float32(0.5)),
            (40, 24, 3, one / np.float32(1)), (40, 24, 0, one / np.float32(2))]
    assert np.array_equal(t.view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
    r50 = P.RigPlan([P.CameraSource((900, 1600), dict(resize=0.44, crop=(0, 140, 704, 396)))]).box2d_table()[0]
    assert r50[:3].tolist() == [704.0, 256.0, 140.0]
    # 1 / resize: one fp32 division of the fp32 resize, as the C entry point's `1.f / resize` on its float argument
    assert r50[3].view(np.uint32) == (one / np.float32(0.44)).view(np.uint32)


def test_key_follows_every_camera():
    base = P.RigPlan(sources())
    assert base.key == P.RigPlan(sources()).key
    other = sources()
    other[1] = P.CameraSource((100, 168), dict(resize=0.25, crop=(1, 1, 41, 25)), "nv12", layout=dict(pitch=192))
    assert P.RigPlan(other).key != base.key
    other = sources()
    other[3] = P.CameraSource((30, 50), dict(resize=1, crop=(5, 3, 45, 27)), "nv12", layout=dict(pitch=54))
    assert P.RigPlan(other).key != base.key
    assert P.RigPlan(sources()[::-1]).key != base.key


def test_rig_entry_point_refuses_before_any_hip_call():
    """The validation runs on the host descriptors alone, so it is checkable without a device."""
    import ctypes
    rig = P.RigPlan(sources())
    cams = rig.descriptors()
    fn = _lib.lib().simpb_preprocess_rig_nhwc4_f16
    one = ctypes.c_void_p(64)
    lens = (sum(k.size for k in rig.kx), 5 * 40, sum(k.size for k in rig.ky), 5 * 24, rig.mid_rows)
    for n_cams, n_images in ((0, 10), (17, 17), (5, 9), (5, 0)):
        assert fn(one, one, one, one, one, one, one, one, one, one, cams, n_cams, n_images, 24, 40, *lens, 1, None) == 1
    assert fn(one, one, one, one, one, one, one, one, one, one, None, 5, 10, 24, 40, *lens, 1, None) == 1
    assert fn(None, one, one, one, one, one, one, one, one, one, cams, 5, 10, 24, 40, *lens, 1, None) == 1
    cams[1].pitch = 167
    assert fn(one, one, one, one, one, one, one, one, one, one, cams, 5, 10, 24, 40, *lens, 1, None) == 1
