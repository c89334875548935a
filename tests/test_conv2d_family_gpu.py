"""GPU (MI355X): the cross-entry bit equalities of tests/test_conv2d_family.py on the device, at the same three shapes."""
import pytest

from test_conv2d_family import SHAPES, check_family

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("H,W", SHAPES)
def test_entry_points_share_one_arithmetic_on_device(H, W):
    check_family(H, W, "cuda")
