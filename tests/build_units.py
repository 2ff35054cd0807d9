"""The build's table of translation units (tactile_gym_amd/csrc/units.txt) for the tests: what is built, into which library, with which flags."""
import os

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tactile_gym_amd", "csrc")
TABLE = os.path.join(CSRC, "units.txt")
BUILD = os.path.join(CSRC, "build.sh")


def rows():
    """[(name, library, flags)] in table order; flags is the text between the library and the comment, '' for none."""
    out = []
    for line in open(TABLE):
        fields = line.split("#", 1)[0].split()
        if fields:
            assert len(fields) >= 2, line
            out.append((fields[0], fields[1], " ".join(fields[2:])))
    return out


def units():
    """{name: (library, flags)}"""
    table = rows()
    assert len({name for name, _, _ in table}) == len(table), "a unit is listed twice"
    return {name: (library, flags) for name, library, flags in table}


def assert_exact_product_unit(name):
    """A unit whose float arithmetic is a bit-exact specification: built, into the product library, with contraction off, and no fast-math anywhere."""
    table = units()
    assert name in table, name
    library, flags = table[name]
    assert "-ffp-contract=off" in flags.split(), (name, flags)
    assert library in ("product", "both"), (name, library)
    assert "fast-math" not in open(TABLE).read() and "fast-math" not in open(BUILD).read()
