"""Checkpoint bridge (scope row f3), SampleRNN half: a pickle WRITTEN BY THE REFERENCE's own lib.save_params
(sampleRNN/lib/__init__.py:96-102, executed by tests/golden/make_ckpt_golden.py) is read by the product's load_params;
and a pickle written by the product is one the reference's load_params (:104-109) reads into its own registry."""
import os
import pickle

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKL = os.path.join(HERE, "golden", "ref_samplernn_ckpt.pkl")


def test_product_loads_reference_written_pickle(tmp_path):
    from parrot_amd.sampleRNN import lib
    with open(PKL, "rb") as f:
        blob = pickle.load(f)
    assert len(blob) == 59 and "BigFrameLevel.GRU1.Step.Input.W0" in blob and "SampleLevel.Embedding" in blob
    lib.delete_all_params()
    lib.set_device("cpu")
    try:
        lib.load_params(PKL)
        named = lib.named_params()
        assert set(named) == set(blob)
        for n, v in blob.items():
            got = named[n].detach().numpy()
            assert got.dtype == np.float32 and got.shape == np.asarray(v).shape, n
            assert np.array_equal(got, np.asarray(v, dtype=np.float32)), n
        # and back out: product writer -> plain pickle of {name: ndarray}, same names, same values
        out = tmp_path / "again.pkl"
        lib.save_params(str(out))
        with open(out, "rb") as f:
            again = pickle.load(f)
        assert set(again) == set(blob)
        for n, v in blob.items():
            assert isinstance(again[n], np.ndarray) and np.array_equal(again[n], np.asarray(v, dtype=np.float32)), n
    finally:
        lib.delete_all_params()


def test_reference_loads_product_written_pickle(tmp_path):
    """The reference's load_params is `pickle.load` followed by `_params[name].set_value(val)` for every entry, on the
    registry whose names and shapes the reference-written fixture carries.  So the product's pickle must unpickle with no
    global but NumPy's (and `_codecs.encode`, which protocol 2 writes for byte strings), and hold every registered name as
    a float32 array of the registered shape, bit for bit.
    (tests/golden/make_ckpt_golden.py also runs the reference's own load_params on it when it regenerates the fixture.)"""
    from parrot_amd.sampleRNN import lib
    with open(PKL, "rb") as f:
        registry = {n: np.asarray(v).shape for n, v in pickle.load(f).items()}
    rng = np.random.RandomState(7)
    fresh = {n: rng.randn(*shape).astype(np.float32) for n, shape in registry.items()}
    path = tmp_path / "product.pkl"
    lib.delete_all_params()
    lib.set_device("cpu")
    try:
        for n, v in fresh.items():
            lib.param(n, v)
        lib.save_params(str(path))
    finally:
        lib.delete_all_params()

    class NumpyOnly(pickle.Unpickler):
        def find_class(self, module, name):
            if module.split(".")[0] != "numpy" and (module, name) != ("_codecs", "encode"):
                raise pickle.UnpicklingError(f"{module}.{name}: not a NumPy class")
            return super().find_class(module, name)
    with open(path, "rb") as f:
        blob = NumpyOnly(f).load()
    assert len(blob) == 59 and set(blob) == set(registry)
    for n, v in fresh.items():
        got = blob[n]
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == v.shape, n
        assert np.array_equal(got, v), n
