"""Engine(library=): a second build of libfheaes.so in one process next to the product's -- what the `so:<path>` A/B mode of the tools
relies on.  The second build here is a byte copy of the product library under another path, which the loader maps a second time:
two libraries with their own contexts and streams on one GPU, the same keys, the same input, word-identical outputs."""
import importlib.util
import shutil
from pathlib import Path

import numpy as np
import pytest

from gpu_support import dev, host, tc  # noqa: F401
from tfhe_aes_amd import PARAM_OPT, PARAM_TOY, _build, _native, aes_clear

spec = importlib.util.spec_from_file_location("tools_measure", Path(__file__).resolve().parent.parent / "tools" / "measure.py")
measure = importlib.util.module_from_spec(spec)
spec.loader.exec_module(measure)

pytestmark = pytest.mark.gpu

BYTES = [0x00, 0x01, 0x53, 0x7F, 0x80, 0xA7, 0xFE, 0xFF, 0x10, 0x3C, 0x52, 0x63, 0x9A, 0xC4, 0xE1, 0x2B]      # test_gpu_tools_measure.py's


def test_two_libraries_in_one_process(toy, tc, tmp_path):
    copy = tmp_path / "libfheaes_copy.so"
    shutil.copyfile(_build.ENGINE_SO, copy)
    other = _native.Engine(PARAM_TOY, device=0, library=copy)
    try:
        other.upload_keys(toy.keys.ksk, toy.keys.bsk, toy.keys.pfpksk)
        default = toy.engine()
        assert other._lib is not default._lib and other._lib._handle != default._lib._handle
        assert default._lib is _native.load_library()
        ct = tc.encrypt_bytes(BYTES)
        outs = []
        for eng in (default, other):
            d = dev(ct)
            eng.sbox(d, len(BYTES), False)
            eng.synchronize()
            outs.append(host(d))
        assert np.array_equal(outs[0], outs[1])
        for out in outs:
            assert list(tc.decrypt_bytes(out)) == [aes_clear.SBOX[v] for v in BYTES]
    finally:
        other.close()


def test_session_hands_the_library_to_the_engine(monkeypatch):
    """needs no GPU: measure.session is PARAM_OPT only, so a stand-in Engine records what its constructor gets"""
    made = []

    class Engine:
        def __init__(self, params, device=0, allow_dev_build=False, library=None):
            made.append({"params": params, "device": device, "allow_dev_build": allow_dev_build, "library": library})

        def upload_keys(self, ksk, bsk, pfpksk):
            made[-1]["keys"] = (ksk, bsk, pfpksk)

    monkeypatch.setattr(measure._native, "Engine", Engine)
    client, eng = measure.session(0xAE50001, 1, 2, library="some/libfheaes.so", allow_dev_build=True)
    assert isinstance(eng, Engine)
    assert {k: made[0][k] for k in ("params", "device", "allow_dev_build", "library")} == \
        {"params": PARAM_OPT, "device": 0, "allow_dev_build": True, "library": "some/libfheaes.so"}
    keys = client.server_keys()
    assert all(a is b for a, b in zip(made[0]["keys"], (keys.ksk, keys.bsk, keys.pfpksk)))
    measure.session(0xAE50001)
    assert made[1]["library"] is None and made[1]["allow_dev_build"] is False
