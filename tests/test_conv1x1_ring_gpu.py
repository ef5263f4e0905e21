"""The ring arm of k_conv1x1_h2 (raw activations by LDS DMA, BN + ReLU + fp16 split on the consumer side) against the tiled
arm and the small-launch kernel on the same input: the same bits in every output value, published range and y-scale.
Shapes: the four dense-block maps and the transitions, odd stage counts, pixel tiles that straddle images, padded plane
strides, a dead-pixel tail and a poisoned image; hw = 49 / 37 and odd plane strides take the tiled arm and must agree too."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

# (cin, cout, hw, n, terms, prologue, x plane pad, y plane pad); every case has >= 512 pixel tiles of 128 (the two-tile size)
CASES = [
    (64, 128, 3136, 21, True, True, 0, 0),        # 56 map, first layer of block 1; 65 856 pixels: a dead-pixel tail
    (224, 128, 3136, 22, False, True, 0, 0),      # 56 map, last layer of block 1
    (128, 128, 784, 85, True, True, 0, 0),        # 28 map
    (80, 128, 784, 85, False, True, 0, 0),        # odd stage count (5 stages)
    (256, 128, 196, 337, True, True, 0, 0),       # 14 map, odd n: tiles straddle images
    (1008, 128, 196, 335, False, True, 0, 0),     # 63 stages, 1008-channel BN table
    (992, 128, 196, 335, True, True, 4, 0),       # padded x planes (xps = hw + 4)
    (512, 128, 49, 1339, True, True, 0, 0),       # 7 map: hw % 4 != 0 -> tiled arm
    (96, 128, 37, 1773, False, True, 0, 0),       # hw = 37 -> tiled arm
    (128, 128, 784, 85, False, True, 3, 5),       # odd x plane stride -> tiled arm; padded y planes
    (256, 128, 784, 85, False, False, 0, 0),      # transition 1 (no prologue, no ReLU)
    (512, 256, 196, 337, False, False, 0, 4),     # transition 2, two output-channel tiles, padded y planes
    (1024, 512, 49, 1339, False, False, 0, 0),    # transition 3 shape on the 7 map (tiled arm)
    (1024, 512, 196, 337, False, False, 8, 0),    # 1024 channels without a prologue, padded x planes
]


def _run(lib, _lib, case, ring, small, bn_offset=False):
    cin, cout, hw, n, terms, prologue, xpad, ypad = case
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(cin * 7 + hw + n)
    ctot = cin + 32
    xps = hw + xpad
    buf = torch.randn(n, ctot, xps, generator=g, device=dev)
    buf *= (10.0 ** torch.randint(-3, 3, (n, 1, 1), generator=g, device=dev).float())
    w = torch.randn(cout, cin, generator=g, device=dev) / cin ** 0.5
    sc = torch.rand(cin, generator=g, device=dev) + 0.5
    sh = torch.randn(cin, generator=g, device=dev) * 0.3
    bias = torch.randn(cout, generator=g, device=dev)
    if bn_offset:                                                      # the same values, 4 bytes into a larger allocation
        sc, sh = (torch.cat([v.new_zeros(1), v])[1:] for v in (sc, sh))
        assert sc.data_ptr() % 16 == 4 and sh.data_ptr() % 16 == 4
    from mirx.model import _split2h_weights
    w2, osc = _split2h_weights(w)
    rng_in = buf[:, :cin, :hw].abs().amax(dim=(1, 2)).contiguous()
    rng_in[1] = float("inf")                                           # a poisoned image
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
    _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_RING, 1 if ring else 0), "set_tuning")
    _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_SMALL_MAX_WG, 1 << 20 if small else 0), "set_tuning")
    yps = hw + ypad
    y = torch.full((n, cout, yps), -7.0, device=dev)
    aux = torch.zeros(n, device=dev)
    ks = float(sc.abs().max()) if prologue else 1.0
    kb = float(sh.abs().max()) if prologue else 0.0
    if terms:
        _lib.check(lib.mirx_conv1x1_bn_relu_split2h_terms(vp(buf), ctot * xps, cin, vp(sc), vp(sh), vp(w2), vp(osc), vp(bias), n,
                                                          hw, vp(y), vp(rng_in), ks, kb, float(w.abs().sum(dim=1).max()),
                                                          float(bias.abs().max()), vp(aux), xps, None), "terms")
    else:
        _lib.check(lib.mirx_conv1x1_bn_relu_split2h(vp(buf), ctot * xps, cin, vp(sc) if prologue else None,
                                                    vp(sh) if prologue else None, vp(w2), vp(osc), vp(bias), n, hw, cout,
                                                    1 if prologue else 0, vp(y), cout * yps, vp(rng_in), ks, kb, vp(aux), xps,
                                                    yps, None), "split2h")
    torch.cuda.synchronize()
    return y.view(torch.int32).clone(), aux.view(torch.int32).clone()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "cin%d_co%d_hw%d_n%d_%s%s_xp%d_yp%d" % (
    c[0], c[1], c[2], c[3], "terms" if c[4] else "fp32", "" if c[5] else "_noprologue", c[6], c[7]))
def test_ring_arm_is_bit_identical_to_the_tiled_arm_and_the_small_kernel(case):
    from mirx import _lib
    lib = _lib.load()
    n, hw, terms, ypad = case[3], case[2], case[4], case[7]
    try:
        outs = [_run(lib, _lib, case, ring, small) for ring, small in ((True, False), (False, False), (False, True))]
    finally:
        _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_RING, 1), "set_tuning")
        _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_SMALL_MAX_WG, 128), "set_tuning")
    clean = [b for b in range(n) if b != 1]
    for other in outs[1:]:
        assert torch.equal(outs[0][0][clean], other[0][clean])
        assert torch.equal(outs[0][1][clean], other[1][clean])
    for y, aux in outs:                                                # the poisoned image: NaN from every arm
        if terms:
            assert bool(torch.isnan(aux.view(torch.float32)[1]))
        else:
            assert bool(torch.isnan(y[1, :, :hw].view(torch.float32)).all())
    # the padding between planes is never written
    if ypad and not terms:
        assert bool((outs[0][0].view(torch.float32)[:, :, hw:] == -7.0).all())


@pytest.mark.parametrize("n,terms", [(2, False), (2, True), (3, False)])
def test_small_launch_falls_back_to_the_tiled_kernel_on_misaligned_bn_vectors(n, terms):
    """The one-wave kernel fills its BN table with 16-byte loads; `scale` / `shift` that are not 16-byte aligned (views 4 bytes
    into a larger allocation) keep the layer on the tiled kernel, which reads them element by element: the same bits as the
    aligned call, which takes the one-wave kernel (7 x 7 map, 512 channels, 2 or 3 images: far below the small-launch limit)."""
    from mirx import _lib
    lib = _lib.load()
    case = (512, 128, 49, n, terms, True, 0, 0)
    try:
        (ya, auxa), (yo, auxo) = (_run(lib, _lib, case, False, True, bn_offset=off) for off in (False, True))
    finally:
        _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_RING, 1), "set_tuning")
        _lib.check(lib.mirx_set_tuning(_lib.TUNE_CONV1X1_SMALL_MAX_WG, 128), "set_tuning")
    clean = [b for b in range(n) if b != 1]                            # image 1 is poisoned (NaN from either kernel)
    assert torch.equal(ya[clean], yo[clean])
    assert torch.equal(auxa[clean], auxo[clean])


def test_ring_switch_validates_its_argument():
    from mirx import _lib
    lib = _lib.load()
    assert lib.mirx_set_tuning(_lib.TUNE_CONV1X1_RING, 2) != 0
    assert lib.mirx_set_tuning(_lib.TUNE_CONV1X1_RING, 1) == 0
