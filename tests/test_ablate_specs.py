"""Every spec of tools/ablate.py still applies to the committed kernel sources (text only: nothing is compiled).  The tool patches by
exact string match, so an edit to the kernel that touches a snippet -- or puts a second copy of one into another file -- breaks a
spec silently until somebody builds it on a GPU day; this is the check that notices at once."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_ablate():
    spec = importlib.util.spec_from_file_location("ablate_tool", os.path.join(ROOT, "tools", "ablate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ablate = load_ablate()


def kernel_sources():
    return {n: open(os.path.join(ablate.CSRC, n)).read() for n in ablate.KERNEL_FILES}


def test_table_is_not_empty_and_names_are_unique():
    names = [name for name, _, _ in ablate._TABLE]
    assert len(names) >= 30 and len(set(names)) == len(names)
    assert set(ablate.SPECS) == set(names)


@pytest.mark.parametrize("spec", sorted(ablate.SPECS))
def test_spec_applies_to_the_committed_sources(spec):
    base = kernel_sources()
    replacements = ablate.SPECS[spec]
    assert replacements
    for old, new in replacements:
        assert old != new, spec
        assert [n for n, t in base.items() if old in t], (spec, old[:60])  # (patch() itself then insists on exactly one file)
    patched = ablate.patch(dict(base), spec)
    assert set(patched) == set(base)
    changed = [n for n in base if patched[n] != base[n]]
    assert changed, spec
    for old, new in replacements:  # every replacement of the spec took effect, not only the first
        assert any(new in patched[n] for n in changed) or new == "", (spec, old[:60])


def test_every_kernel_fragment_is_patched_from():
    """KERNEL_FILES lists what warp_rows.h includes: a fragment that is missing there would be compiled unpatched from the wrong place."""
    text = open(os.path.join(ablate.CSRC, "warp_rows.h")).read()
    included = {ln.split('"')[1] for ln in text.splitlines() if ln.strip().startswith('#include "rows_')}
    assert included and included <= set(ablate.KERNEL_FILES)
    for n in ablate.KERNEL_FILES:
        assert os.path.isfile(os.path.join(ablate.CSRC, n)), n


def test_unknown_spec_is_refused():
    with pytest.raises(SystemExit):
        ablate.patch(kernel_sources(), "no_such_spec")


def test_docstring_lists_exactly_the_table():
    listed = [ln.split()[0] for ln in ablate.__doc__.split("The specs")[1].splitlines()[2:] if ln.startswith("    ")]
    assert listed == [name for name, _, _ in ablate._TABLE]
