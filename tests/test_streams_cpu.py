"""The table of the stream-contract tests (tests/stream_cases.py) names every launching entry point of the eight training
bindings: a new entry point cannot escape the harness unnoticed.  No library and no GPU are needed."""
import pytest

from tests import stream_cases as sc

FAMILIES = ("pg", "pr", "pa", "pm", "ps", "pn", "po", "pt")


def test_the_eight_families_are_listed():
    assert tuple(sc.signatures()) == FAMILIES == tuple(sc.NON_LAUNCHING)
    assert {e.family for e in sc.ENTRIES} == set(FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_every_entry_point_is_in_the_table_or_listed_as_not_launching(family):
    names = sc.signatures()[family]
    covered = {n for e in sc.ENTRIES if e.family == family for n in e.covers}
    quiet = set(sc.NON_LAUNCHING[family])
    assert covered <= names, f"{family}: the table names entry points the binding does not have: {sorted(covered - names)}"
    assert quiet <= names, f"{family}: listed as not launching but not in the binding: {sorted(quiet - names)}"
    assert not covered & quiet, f"{family}: both launched and listed as not launching: {sorted(covered & quiet)}"
    missing = names - covered - quiet
    assert not missing, f"{family}: entry points outside the stream harness: {sorted(missing)} (tests/stream_cases.py)"


def test_only_queries_and_the_host_function_are_exempt():
    """The explicit list holds nothing but the version, the error text, the size / geometry queries and pm_assign."""
    for family, quiet in sc.NON_LAUNCHING.items():
        for n in quiet:
            assert n in ("abi_version", "last_error", "geometry", "table_check") or n.endswith(("_bytes", "_ranges", "_slab_rows")) \
                or (family, n) == ("pm", "assign"), (family, n)


def test_entries_are_well_formed():
    assert len(set(sc.ENTRY_IDS)) == len(sc.ENTRIES)
    assert {e.family for e in sc.PAIR_ENTRIES} == {"pa", "pm", "ps", "pg"}
    assert all(e.caches_scratch == (e.family != "pg") for e in sc.PAIR_ENTRIES)
    assert len({sc.SEED_A, sc.SEED_B, *sc.PAIR_SEEDS}) == 6
