"""LSTM decoders with bf16 weight slabs on the decode machine (ParrotSampleDesc::bf16, plans_decode.hip build_persist_lstm,
plans_common.h pm_place): planned and replayed symbolically on the CPU -- no device memory is touched.  A bf16 slab is
charged half the LDS of an f32 one, so slabs that streamed become resident; configurations the bf16 machine does not
take get no plan at all."""
import ctypes as C

from parrot_amd import _lib
from tests.test_decode_plan_cpu import _desc, _plan


def _lstm(bf16, **kw):
    d = _desc(**kw)
    d.cell, d.bf16 = 1, bf16
    for l in range(d.L):
        d.Wg_t16[l] = 0x7100_0000_0000 if bf16 else None  # never dereferenced by the dry run
    return d


def test_configs2_width_keeps_every_layer_slab_resident():
    """2 x 1024, E = 512, B = 16: layer 1 has K = 2560 > the 2304 f32 K-rows a workgroup holds; as bf16 both layers' slabs
    fit together (20480 + 12800 of 36864 floats).  Only the four f32 output tiles (K = 2560) still stream."""
    kw = dict(L=2, H=1024, E=512, B=16, fb=(0,))
    rc, info = _plan(_lstm(1, **kw))
    assert rc == 0 and info[2] == 0, (rc, info)
    assert info[0] == 4 and info[13] == 1
    assert info[14] <= 4, info
    rc32, info32 = _plan(_lstm(0, **kw))
    assert rc32 == 0 and info32[2] == 0
    assert info32[14] > info[14], (info32[14], info[14])
    assert info32[:14] == info[:14]           # the same phases and units: only the residency differs


def test_cfg4_width_streams_fewer_units_than_its_f32_plan():
    """3 x 1536, E = 256, B = 16: 384 tiles per layer on 256 workgroups (two units per workgroup and phase).  The f32 plan
    keeps 256 layer-0 slabs on chip (900 of 1156 units stream); with bf16 slabs a workgroup holds two layer-0 slabs or
    one layer-1 slab."""
    kw = dict(L=3, H=1536, E=256, R=1536, B=16, fb=(0,))
    rc, info = _plan(_lstm(1, **kw))
    assert rc == 0 and info[2] == 0, (rc, info)
    assert info[13] == 2
    rc32, info32 = _plan(_lstm(0, **kw))
    assert rc32 == 0 and info32[13] == 2
    assert info[14] < info32[14], (info[14], info32[14])


def test_padding_rows_and_empty_k_ranges_plan():
    """The widths of the GPU tests: H = 64, E = 32 with 64 fed-back rows is 5 steps of 32 for 8 waves."""
    rc, info = _plan(_lstm(1, L=3, H=64, E=32, R=48, B=5, S=14, fb=(0, 1, 2), speaker=True))
    assert rc == 0 and info[2] == 0 and info[14] == 0, (rc, info)


def test_what_the_bf16_machine_does_not_take_is_refused():
    ok = dict(L=2, H=64, E=32, R=48, B=16, S=10, fb=(0,))
    assert _plan(_lstm(1, **ok))[0] == 0
    rc, _ = _plan(_lstm(1, **dict(ok, H=48)))             # K steps are 32 deep
    assert rc != 0
    rc, _ = _plan(_lstm(1, **dict(ok, E=48)))
    assert rc != 0
    d = _lstm(1, **ok)
    d.cell = 0                                             # GRU programs have no bf16 units
    assert _plan(d)[0] != 0
    d = _lstm(1, **ok)
    d.gmm_K = 3
    assert _plan(d)[0] != 0
    d = _lstm(1, **ok)
    d.layer_norm = 1
    assert _plan(d)[0] != 0
    d = _lstm(1, **dict(ok, B=65))
    assert _plan(d)[0] != 0
    d = _lstm(1, **ok)
    d.Wg_t16[1] = None                                     # a layer without its bf16 copy
    assert _plan(d)[0] != 0


def test_size_query_is_zero_for_what_is_refused():
    lib = _lib.load()
    d = _lstm(1, L=2, H=48, E=32, R=48, B=16, S=10, fb=(0,))
    assert lib.parrot_sample_persist_floats(C.byref(d)) == 0
    d = _lstm(1, L=2, H=64, E=32, R=48, B=16, S=10, fb=(0,))
    d.cell = 0
    assert lib.parrot_sample_persist_floats(C.byref(d)) == 0
