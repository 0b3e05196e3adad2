"""CPU: fused.Knobs, the declared table of FusedStep's tuning values (no FusedStep is built)."""
import dataclasses

import pytest

# the selectors of the deleted kernel variants, gone from nof_field_desc and never knobs. Written as
# (stem, tail) so that a search of the tree for a stale use of one of them finds none, this list included
REMOVED = tuple(f"{stem}_{tail}" for stem, tail in (
    ("blocks_per", "cu"), ("scatter_waves_per", "ray"), ("scatter_ls", "levels"), ("scatter", "kernel"),
    ("encode", "sigma"), ("scatter", "flat"), ("mlp_pass1", "tiles"), ("scatter_fuse", "levels"), ("encode", "wpb")))


def test_every_knob_changes_the_graph_key_part():
    """FusedStep._graph_key hashes dataclasses.astuple(knobs): changing any single field must change
    it, or a captured graph would replay with the old kernel shape."""
    from bundlesdf_amd.fused import Knobs
    base = dataclasses.astuple(Knobs())
    fields = dataclasses.fields(Knobs)
    assert len(fields) == len(base) == 11
    for f in fields:
        k = Knobs()
        old = getattr(k, f.name)
        setattr(k, f.name, (not old) if isinstance(old, bool) else old + 1)
        assert dataclasses.astuple(k) != base, f.name


def test_undeclared_knob_is_an_error():
    from bundlesdf_amd.fused import Knobs
    k = Knobs()
    with pytest.raises(AttributeError):
        k.scater_slots = 256
    with pytest.raises(TypeError):
        dataclasses.replace(k, scater_slots=256)


def test_descriptor_knobs_are_descriptor_fields():
    from bundlesdf_amd import _lib
    from bundlesdf_amd.fused import Knobs
    desc = {f[0] for f in _lib.FieldDesc._fields_}
    knobs = {f.name for f in dataclasses.fields(Knobs)}
    assert Knobs.DESCRIPTOR and len(set(Knobs.DESCRIPTOR)) == len(Knobs.DESCRIPTOR)
    for name in Knobs.DESCRIPTOR:
        assert name in knobs and name in desc, name
    # a knob that is a descriptor field of the same name must be marked, or it would never reach the library
    assert (knobs & desc) == set(Knobs.DESCRIPTOR)
    for name in REMOVED:
        assert name not in desc and name not in knobs, name
