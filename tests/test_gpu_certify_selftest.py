"""The certificate kernels against the plain host evaluation of their definitions (csrc/certify_selftest.hpp):
arenas and tables built on the host, clean and with planted errors, in both orders; every counter of every
case must equal the host's, at 1, 63 .. 65, 255 .. 257 states, 3000 states on a grid of two workgroups and a
level of 65536. The planted out-of-range parent ranks must be counted and never loaded."""
import pytest

pytestmark = pytest.mark.gpu
sr = pytest.importorskip("stateright_amd")
from stateright_amd import _native as N  # noqa: E402


def test_certificate_kernels_match_the_host_evaluation():
    assert N.load().sr_selftest_certify_gpu(0) == 0, N.last_error()
