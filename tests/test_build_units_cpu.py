"""The build of the two HIP libraries (tactile_gym_amd/csrc: units.txt, build.sh, relink.sh) without a compiler: the table against the directory,
build.sh's dry run against the table and against the two link orders of record, relink.sh's link line, the job limit, and a failed unit."""
import glob
import os
import stat
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import build_units  # noqa: E402

CSRC = build_units.CSRC
COMMON = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value"
LINK = "--offload-arch=gfx950 -shared -fPIC"
# the link orders of the build before it read a table, object by object: where a unit's code object sits in the library shows in the step rate
PRODUCT_ORDER = ("tg_raster tg_noise tg_api tg_contact_wave tg_scene tg_exchange tg_fused tg_broadphase tg_api_state tg_api_ops tg_spin tg_stack "
                 "tg_augment tg_rollout tg_replay tg_affine tg_vecnorm tg_action_head tg_conv_stem tg_loss_head tg_sac_loss tg_mlp tg_conv tg_api_obs").split()
TEST_ORDER = "tg_narrow_test tg_selftest tg_render_test tg_scene_test tg_stack_test tg_physics_test tg_state_test tg_raster tg_scene tg_stack".split()
CONTRACT_OFF = {"tg_raster", "tg_noise", "tg_scene", "tg_selftest", "tg_broadphase", "tg_augment", "tg_rollout", "tg_replay", "tg_affine",
                "tg_vecnorm", "tg_action_head", "tg_conv_stem", "tg_loss_head", "tg_sac_loss", "tg_mlp", "tg_conv"}


def _script(name, tmp_path, env=None, path_first=None):
    """Run csrc/<name> with a clean set of the build's variables; (exit status, stdout lines, stderr)."""
    e = {k: v for k, v in os.environ.items() if k not in ("HIPCC", "TG_OUT", "TG_EXTRA_FLAGS", "TG_INCREMENTAL", "TG_JOBS", "TG_DRY_RUN", "MAX_JOBS")}
    e.update({"HIPCC": "HIPCC", "TG_OUT": str(tmp_path / "out")}, **(env or {}))
    if path_first:
        e["PATH"] = str(path_first) + os.pathsep + e["PATH"]
    r = subprocess.run(["bash", os.path.join(CSRC, name)], env=e, capture_output=True, text=True, cwd=str(tmp_path))
    return r.returncode, r.stdout.splitlines(), r.stderr


def _executable(path, text):
    path.write_text(text)
    path.chmod(path.stat().st_mode | stat.S_IXUSR)
    return path


@pytest.fixture(scope="module")
def dry(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dry")
    rc, lines, err = _script("build.sh", tmp, {"TG_DRY_RUN": "1", "TG_JOBS": "5"})
    assert rc == 0 and err == "", err
    assert not (tmp / "out").exists()                                    # a dry run runs nothing
    return str(tmp / "out"), lines


def test_table_and_directory_agree():
    names = [name for name, _, _ in build_units.rows()]
    sources = sorted(os.path.basename(p)[:-len(".hip")] for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert sorted(names) == sources                                      # every unit once, every name with its file
    assert all(library in ("product", "test", "both") for _, library, _ in build_units.rows())
    assert len(build_units.units()) == 31


def test_flagged_set():
    table = build_units.units()
    assert {name for name, (_, flags) in table.items() if flags} == CONTRACT_OFF
    assert {flags for _, flags in table.values()} == {"", "-ffp-contract=off"}
    assert table["tg_narrow_test"] == ("test", "")                       # it switches contraction off by pragma


def test_dry_run_compiles_every_unit_with_its_flags(dry):
    out, lines = dry
    assert lines[0] == "# at most 5 compilers at a time"
    compiles = sorted(lines[1:-2])
    want = sorted(" ".join(["HIPCC", COMMON] + ([flags] if flags else []) + ["-c", f"{name}.hip", "-o", f"{out}/{name}.o"])
                  for name, (_, flags) in build_units.units().items())
    assert compiles == want


def test_dry_run_links_in_the_orders_of_record(dry):
    out, lines = dry
    for line, order, lib in ((lines[-2], PRODUCT_ORDER, "libtactile_gym_hip.so"), (lines[-1], TEST_ORDER, "libtactile_gym_hip_test.so")):
        assert line == " ".join(["HIPCC", LINK] + [f"{out}/{name}.o" for name in order] + ["-o", f"{out}/{lib}"])
    # ... which is what the table says: its order, product and both / test then both
    rows = build_units.rows()
    assert [n for n, library, _ in rows if library in ("product", "both")] == PRODUCT_ORDER
    assert [n for n, library, _ in rows if library == "test"] + [n for n, library, _ in rows if library == "both"] == TEST_ORDER
    assert [n for n, _, _ in rows][2:4] == ["tg_api", "tg_contact_wave"]     # the long compiles start at once under any limit of 4 or more


def test_relink_dry_run_is_the_product_link_line(dry, tmp_path):
    out, lines = dry
    rc, relink, err = _script("relink.sh", tmp_path, {"TG_DRY_RUN": "1", "TG_OUT": out})
    assert (rc, err) == (0, "") and relink == [lines[-2]]


@pytest.mark.parametrize("jobs", ["0", "abc", "-3", "2x"])
def test_job_limit_is_a_positive_number(tmp_path, jobs):
    rc, lines, err = _script("build.sh", tmp_path, {"TG_DRY_RUN": "1", "TG_JOBS": jobs})
    assert rc != 0 and lines == [] and "TG_JOBS" in err and repr(jobs) in err


def test_job_limit_default(tmp_path):
    bin_ = tmp_path / "bin"
    bin_.mkdir()
    nproc = _executable(bin_ / "nproc", "#!/bin/sh\necho 192\n")
    assert _script("build.sh", tmp_path, {"TG_DRY_RUN": "1"}, bin_)[1][0] == "# at most 16 compilers at a time"
    assert _script("build.sh", tmp_path, {"TG_DRY_RUN": "1", "MAX_JOBS": "12"}, bin_)[1][0] == "# at most 12 compilers at a time"
    assert _script("build.sh", tmp_path, {"TG_DRY_RUN": "1", "MAX_JOBS": "12", "TG_JOBS": "3"}, bin_)[1][0] == "# at most 3 compilers at a time"
    nproc.write_text("#!/bin/sh\necho 6\n")
    assert _script("build.sh", tmp_path, {"TG_DRY_RUN": "1"}, bin_)[1][0] == "# at most 6 compilers at a time"


@pytest.mark.parametrize("jobs", ["1", "4", "64"])
def test_a_failed_unit_fails_the_build_before_any_link(tmp_path, jobs):
    log = tmp_path / "log"
    stub = _executable(tmp_path / "stub_cc", '#!/bin/bash\necho "$*" >> "$STUB_LOG"\ncase "$*" in *"-c tg_stack.hip"*) exit 7 ;; esac\n')
    rc, lines, _ = _script("build.sh", tmp_path, {"HIPCC": str(stub), "STUB_LOG": str(log), "TG_JOBS": jobs})
    ran = log.read_text().splitlines()
    assert rc == 7 and not any("built" in line for line in lines)
    assert any("-c tg_stack.hip" in line for line in ran) and not any("-shared" in line for line in ran)
    # ... and with a compiler that succeeds, every unit is compiled once and both libraries are linked
    log.unlink()
    stub.write_text('#!/bin/bash\necho "$*" >> "$STUB_LOG"\n')
    rc, lines, _ = _script("build.sh", tmp_path, {"HIPCC": str(stub), "STUB_LOG": str(log), "TG_JOBS": jobs})
    ran = log.read_text().splitlines()
    assert rc == 0 and lines[-1].startswith("built ")
    assert sorted(line.split(" -c ")[1].split(".hip")[0] for line in ran[:-2]) == sorted(build_units.units())
    assert [line.split()[-1].rsplit("/", 1)[1] for line in ran[-2:]] == ["libtactile_gym_hip.so", "libtactile_gym_hip_test.so"]
