"""The Iris checker (oracle/iris_oracle.c) off the default configuration, by hand: tests/test_gpu_iris_configs.py holds the GPU to
it at 16 beams, 40 x 180 and 10 x 100 x 3, so these known answers check the reference there first.  No GPU."""
import numpy as np

import oracle_iris_binding as oi


def _cloud(pts):
    c = np.zeros((len(pts), 8), np.float32)
    c[:, :3] = np.asarray(pts, np.float32)
    return c


def test_image_known_answers_with_16_beams():
    """elevation bit floor((atan2(z, dis) deg + 15) / 4), clamped to [0, 7] (D.h:538-558)"""
    cfg = oi.config(nscan=16)
    img, key = oi.make_image(cfg, _cloud([[10.0, 0.0, 0.0]]))
    assert img[10, 180] == 1 << 3 and np.count_nonzero(img) == 1 and not key.any()        # (0 + 15) / 4 = 3.75 -> bit 3
    t = lambda deg: 10.0 * np.tan(np.radians(deg))
    for deg, bit in ((-20.0, 0), (-15.5, 0), (-14.0, 0), (-10.5, 1), (4.5, 4), (12.5, 6), (14.0, 7), (16.9, 7), (20.0, 7)):
        img, _ = oi.make_image(cfg, _cloud([[0.0, -10.0, t(deg)]]))                      # yaw -90 + 180 = column 90
        assert img[10, 90] == 1 << bit and np.count_nonzero(img) == 1, (deg, bit, img[10, 90])
    img64, _ = oi.make_image(oi.config(), _cloud([[0.0, -10.0, t(-20.0)]]))
    assert img64[10, 90] == 1 << 1                                                        # 64 beams: (-20 + 24.9) / 4 = 1.2 -> bit 1


def test_image_known_answers_at_40x180():
    """yaw bin floor(atan2(y, x) deg + 180 + 0.5) runs to 360 whatever `cols` is: with 180 columns everything from yaw -0.5 degrees
    upwards clamps into column 179; the range clamps at row 39"""
    cfg = oi.config(rows=40, cols=180)
    at = lambda deg, d=10.0, z=0.0: [d * np.cos(np.radians(deg)), d * np.sin(np.radians(deg)), z]
    for deg, col in ((100.0, 179), (0.0, 179), (-0.4, 179), (-1.2, 179), (-1.6, 178), (-90.0, 90), (-179.8, 0), (179.9, 179)):
        img, _ = oi.make_image(cfg, _cloud([at(deg)]))
        assert img[10, col] == 1 << 6 and np.count_nonzero(img) == 1, (deg, col, np.argwhere(img))
    img, key = oi.make_image(cfg, _cloud([at(-90.0, 39.99, 1.0), at(-90.0, 40.0, 2.0), at(-90.0, 500.0, 3.0)]))
    assert np.count_nonzero(img) == 1 and img[39, 90] != 0 and key[39] == np.float32(3.0) / np.float32(180) and not key[:39].any()


def test_templates_and_hamming_at_10x100x3():
    """60 template rows (not a multiple of 32): sizes, a rolled copy is found at its shift with distance 0, and the distance of a
    pair with a single unmasked image row counts the unmasked bits only"""
    cfg = oi.config(rows=10, cols=100, nscale=3)
    rs = np.random.RandomState(3)
    a = (rs.random_sample((10, 100)) < 0.4).astype(np.uint8) * rs.randint(1, 255, size=(10, 100)).astype(np.uint8)
    Ta, Ma = oi.encode(cfg, a)
    assert Ta.shape == (60, 100) and set(np.unique(Ta)) <= {0, 255} and set(np.unique(Ma)) <= {0, 255}
    Tz, Mz = oi.encode(cfg, np.zeros_like(a))
    assert not Tz.any() and Mz.all()
    assert oi.hamming(cfg, Ta, Ma, Ta, Ma, 0) == (0.0, 0)
    for sh in (1, 5, 17, 64, 99):
        Tb, Mb = oi.encode(cfg, np.roll(a, sh, axis=1))
        assert oi.hamming_all(cfg, Ta, Ma, Tb, Mb) == (0.0, sh)
        assert oi.hamming(cfg, Ta, Ma, Tb, Mb, sh + 1) == (0.0, sh)
        d, b = oi.hamming(cfg, Ta, Ma, Tb, Mb, sh + 3)
        assert b != sh and d > 0.0
    one = np.zeros_like(a); one[9] = a[9]
    other = np.zeros_like(a); other[9] = a[9] ^ ((rs.random_sample(100) < 0.3) * 0x24).astype(np.uint8)
    T1, M1 = oi.encode(cfg, one); T2, M2 = oi.encode(cfg, other)
    assert M1[[r for r in range(60) if r % 10 != 9]].all()                                # only template rows 9, 19, ..., 59 carry anything
    valid = (M1 | M2) == 0
    d, b = oi.hamming(cfg, T1, M1, T2, M2, 0)
    best = min(np.float32(np.count_nonzero((np.roll(T1, s, axis=1) != T2) & ((np.roll(M1, s, axis=1) | M2) == 0))) /
               np.float32(np.count_nonzero((np.roll(M1, s, axis=1) | M2) == 0)) for s in range(-2, 3))
    assert 0 < np.count_nonzero(valid) <= 600 and np.float32(d) == best
