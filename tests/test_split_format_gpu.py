"""GPU (MI355X): the bit equalities of tests/test_split_format.py on the device, on the same patterns and shapes."""
import pytest

from test_split_format import VOLUME_CASES, check_roundings, check_volume_store

pytestmark = pytest.mark.gpu


def test_both_roundings_match_their_host_mirrors_and_each_other_on_device():
    check_roundings("cuda")


@pytest.mark.parametrize("H,W,scale", VOLUME_CASES)
def test_volume_store8_in_its_four_kernels_on_device(H, W, scale):
    check_volume_store(H, W, scale, "cuda")
