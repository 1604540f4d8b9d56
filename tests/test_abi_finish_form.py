"""CPU checks of kth_ctx_last_finish_form and KTH_HOOK_FINISH_SLICES
(include/kth.h): the argument checks that precede any device work, and the
header's constants against the Python binding's."""
import ctypes
import os
import re

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def lib():
    import kselect
    return kselect.LIB


def _defines(prefix):
    text = open(os.path.join(REPO, "include", "kth.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(" + prefix + r"\w+)\s+(-?\d+)\s*$", text, re.M)}


def test_null_arguments_are_refused(lib):
    import kselect
    form = ctypes.c_int(-7)
    assert lib.kth_ctx_last_finish_form(None, ctypes.byref(form)) == kselect.KTH_EINVAL
    assert lib.kth_ctx_last_finish_form(None, None) == kselect.KTH_EINVAL
    assert form.value == -7  # nothing written
    for value in (0, 1):
        assert lib.kth_ctx_test_hook(None, kselect.KTH_HOOK_FINISH_SLICES, value) == kselect.KTH_EINVAL


def test_constants_match_the_header():
    import kselect
    hooks = _defines("KTH_HOOK_")
    assert hooks["KTH_HOOK_FINISH_SLICES"] == kselect.KTH_HOOK_FINISH_SLICES
    assert sorted(hooks.values()) == list(range(1, len(hooks) + 1)), hooks  # distinct, and the next free id
    assert hooks["KTH_HOOK_FINISH_SLICES"] == len(hooks)
    forms = _defines("KTH_FINISH_")
    assert forms == {"KTH_FINISH_NONE": kselect.KTH_FINISH_NONE, "KTH_FINISH_COUNTS": kselect.KTH_FINISH_COUNTS,
                     "KTH_FINISH_SLICES": kselect.KTH_FINISH_SLICES, "KTH_FINISH_GROUPED": kselect.KTH_FINISH_GROUPED,
                     "KTH_FINISH_LEVELS": kselect.KTH_FINISH_LEVELS}
    assert sorted(forms.values()) == list(range(5))


def test_wrapper_exposes_the_getter():
    import kselect
    assert callable(getattr(kselect.Selector, "finish_form"))
    from kselect._lib import PROTOS
    assert "kth_ctx_last_finish_form" in PROTOS
