"""The pickers of bev_amd/csrc/launch_pick.h without a device (tests/launch_pick_driver.cpp, g++ under the sanitizers): every kernel unit
turns its runtime words into a template instance through them, so a picker that runs its callable twice, not at all or with the wrong
constant launches the wrong kernel.  Each picker over every listed value and over -1, one past the last listed value and INT_MAX."""
import pytest

from tests import hostplan

INT_MAX = 2**31 - 1
# picker number of the driver -> its list, in the header's order: a word that is not listed takes the LAST entry
LISTS = {0: (0, 1), 1: (1, 2, 3, 4, 5), 2: (0, 1, 2, 3, 4), 3: (1, 0), 4: (2, 1, 0), 5: (7,), 6: (1, 2, 3, 4)}
FLAG, PIXEL = 7, 8


@pytest.fixture(scope="module")
def driver():
    return hostplan.build_driver(source="launch_pick_driver.cpp")


def probes(listed):
    return sorted(set(listed) | {-1, max(listed) + 1, listed[-1] + 1, INT_MAX})


@pytest.mark.parametrize("picker", sorted(LISTS))
def test_value_picker_runs_once_with_the_listed_value_or_the_last(driver, picker):
    listed = LISTS[picker]
    words = probes(listed)
    out = hostplan.run_driver(driver, ["%d %d" % (picker, w) for w in words])
    assert out == [[1, w if w in listed else listed[-1]] for w in words]


def test_flag_picker_is_true_for_any_non_zero_word(driver):
    words = [0, 1, 2, -1, INT_MAX, -INT_MAX - 1]
    out = hostplan.run_driver(driver, ["%d %d" % (FLAG, w) for w in words])
    assert out == [[1, int(w != 0)] for w in words]


def test_pixel_picker_is_uint8_for_zero_and_float_otherwise(driver):
    words = [0, 1, 2, -1, INT_MAX]
    out = hostplan.run_driver(driver, ["%d %d" % (PIXEL, w) for w in words])
    assert out == [[1, int(w != 0)] for w in words]  # (the driver's 0 = uint8_t, 1 = float)
