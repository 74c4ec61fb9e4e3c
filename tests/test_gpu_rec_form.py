"""GPU (MI355X): the partial rounds' assembly form dot4_add_uc (csrc/imt_mont_asm_rec.hpp) through the test-only
harness tests/native/rec_form.hip, bit for bit against the Python model of tests/test_rec_form.py on the same corner
corpus (constants in SGPRs, one set per wave)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_rec_form import CSRC, NL, ROOT, SRC, _p, corpus, expected

pytestmark = pytest.mark.gpu


def test_dot4_add_uc_assembly_matches_model():
    so = os.path.join(ROOT, "tests", "native", "librecform.so")
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("imt_device.hpp", "imt_consts.hpp", "imt_mont_asm.hpp",
                                                    "imt_mont_asm_rec.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-I", CSRC, "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    uni, lanes = corpus(n_blocks=96, seed=0x6D04)
    want, _ = expected(uni, lanes)
    out = np.zeros((lanes.shape[0], NL), np.uint32)
    rc = lib.rec_form_gpu(_p(np.ascontiguousarray(lanes)), _p(np.ascontiguousarray(uni)), _p(out),
                          ctypes.c_uint(lanes.shape[0]))
    assert rc == 0
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} lanes differ, first {bad[:8].tolist()}"
