"""docs/SWITCHES.md lists exactly the GRT_* names the package and bench.py read from the environment."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
# getenv("GRT_X") (C++ getenv / std::getenv, Python os.getenv), os.environ.get("GRT_X"...) and
# os.environ["GRT_X"]; macros such as GRT_DEVICE_CHECK never appear as a quoted argument of these
READ = re.compile(r"""(?:getenv\(|environ\.get\(|environ\[)\s*["'](GRT_[A-Z0-9_]+)["']""")
ROW = re.compile(r"^\|\s*`(GRT_[A-Z0-9_]+)`\s*\|", re.M)


def switches_read():
    files = [ROOT / "bench.py"]
    for ext in ("py", "hip", "cpp", "h"):
        files += sorted((ROOT / "gke_ray_train_amd").rglob(f"*.{ext}"))
    names = set()
    for f in files:
        names.update(READ.findall(f.read_text()))
    return names


def test_switch_table_matches_the_environment_reads():
    rows = ROW.findall((ROOT / "docs" / "SWITCHES.md").read_text())
    assert len(rows) == len(set(rows)), sorted(n for n in set(rows) if rows.count(n) > 1)
    read = switches_read()
    assert read, "the scan found no environment reads"
    assert set(rows) == read, {"undocumented": sorted(read - set(rows)), "stale rows": sorted(set(rows) - read)}
