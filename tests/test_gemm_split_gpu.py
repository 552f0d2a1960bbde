"""The split-operand GEMM family through the C ABI (tests/gemm_split_run.py) on the cases of tests/gemm_split_cases.py
(tests/test_gemm_split_cpu.py proves those): exact expected values with ``array_equal`` on every kernel the launcher can
reach, poisoned workspaces and guard rows, the packed path, every variant and switch against the same bits, the non-finite
contract with and without the clamp, and the argument checks.  The default mode (f16x3) runs here; bf16x3 and the one-plane
fp16 mode run the whole list once each in a child process.  No tolerance anywhere.  Needs a real MI355X: -m gpu."""
import os
import subprocess
import sys

import pytest
import torch

import gemm_split_cases as C
import gemm_split_run as R
from myrtlespeech_amd import _lib

pytestmark = pytest.mark.gpu

INVALID, WORKSPACE = 1, 3
RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_split_run.py")


@pytest.fixture(autouse=True)
def default_mode():
    assert R.mode() == "f16x3", "run this file without MS_PRECISION: the other modes run in children"


@pytest.mark.parametrize("c", C.cases(), ids=C.tag)
def test_every_family_is_exact_on_every_variant_and_the_packed_path(lib, c):
    R.check_case(lib, c)


@pytest.mark.parametrize("i", range(len(C.nonfinite_cases())),
                         ids=lambda i: C.tag(C.nonfinite_cases()[i][0]) + "-variant%d-%s" % C.nonfinite_cases()[i][1][:2])
def test_a_non_finite_operand_stays_non_finite_in_its_row_or_column(lib, i):
    R.check_nonfinite(lib, *C.nonfinite_cases()[i])


# ----------------------------------------------------------------------------- the other precision modes
def child(precision, jobs, seconds):
    env = dict(os.environ, MS_PRECISION=precision)
    r = subprocess.run([sys.executable, RUNNER] + jobs, env=env, capture_output=True, text=True, timeout=seconds)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (precision, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_whole_list_with_bf16_planes():
    child("bf16x3", ["exact", "nonfinite"], 900)


def test_whole_list_with_one_fp16_plane():
    child("fp16", ["exact", "nonfinite"], 900)


# ----------------------------------------------------------------------------- the ABI
def test_bad_arguments_are_refused_and_nothing_is_written(lib):
    M, K, N = 70, 64, 36
    x, w, b = C.make("hi", M, K, N, "f16x3")
    call = R.Call(lib, x, w, b)
    P, S = _lib.ptr, _lib.stream_ptr()
    xo = call.xbuf[R.PAD + 1:R.PAD + 1 + M * K].view(M, K)              # one float in: not 16-byte aligned
    wo = call.wbuf[R.PAD + 1:R.PAD + 1 + N * K].view(N, K)
    assert xo.data_ptr() % 16 == 4 and wo.data_ptr() % 16 == 4
    nws = call.nws
    packed = R.scratch(lib.ms_linear_split_packed_bytes(K, N))
    xws = C.x_workspace_bytes(M, K)

    def forward(x_=call.x, w_=call.w, k=K, act=_lib.ACT_NONE, ws_bytes=nws):
        return lib.ms_linear_split_forward(P(x_), P(w_), P(call.b), P(call.out.y), M, k, N, act, 0.0, 1.0, P(call.ws), ws_bytes, S)

    def forward_packed(x_=call.x, k=K, act=_lib.ACT_NONE, ws_bytes=xws):
        return lib.ms_linear_split_forward_packed(P(x_), P(packed), P(call.b), P(call.out.y), M, k, N, act, 0.0, 1.0, P(call.ws),
                                                  ws_bytes, S)
    attempts = (("K % 32", forward(k=48), INVALID), ("K % 32 packed", forward_packed(k=48), INVALID),
                ("misaligned x", forward(x_=xo), INVALID), ("misaligned w", forward(w_=wo), INVALID),
                ("misaligned x packed", forward_packed(x_=xo), INVALID),
                ("short workspace", forward(ws_bytes=nws - 1), WORKSPACE), ("short workspace packed", forward_packed(ws_bytes=xws - 1), WORKSPACE),
                ("act 2", forward(act=2), INVALID), ("act -1", forward(act=-1), INVALID), ("act 2 packed", forward_packed(act=2), INVALID),
                ("pack K % 32", lib.ms_linear_split_pack(P(call.w), P(packed), 48, N, S), INVALID),
                ("pack misaligned w", lib.ms_linear_split_pack(P(wo), P(packed), K, N, S), INVALID))
    torch.cuda.synchronize()
    for name, rc, want in attempts:
        assert rc == want, (name, rc, lib.ms_last_error().decode())
    call.out.untouched("refused calls")
    assert bool((call.ws == 0xFF).all()) and bool((packed == 0xFF).all()), "a refused call wrote to its workspace"
    # ... and the same buffers serve a good call afterwards
    R.exact(call.forward(None, "after the refusals"), C.expected(x, w, b, "f16x3"), "after the refusals")


def test_size_queries(lib):
    for M, K, N in ((1, 32, 1), (3, 32, 5), (70, 64, 36), (3330, 640, 3330)):
        assert lib.ms_linear_split_workspace_bytes(M, K, N) == C.workspace_bytes(M, K, N)
        assert lib.ms_linear_split_packed_bytes(K, N) == C.packed_bytes(K, N)
    for bad in (0, -1):
        assert lib.ms_linear_split_workspace_bytes(bad, 32, 5) == 0 and lib.ms_linear_split_workspace_bytes(3, 32, bad) == 0
        assert lib.ms_linear_split_packed_bytes(bad, 5) == 0 and lib.ms_linear_split_packed_bytes(32, bad) == 0
