"""CPU: lipasr/knobs.py is the one table of the project's LIPASR_* environment variables, the one place the package reads them, and
what README.md shows."""
import glob
import os
import re

import pytest

from lipasr import knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "asr-using-robust-nn_amd")
NAMES = {row.name for row in knobs.TABLE}


def _sources():
    return sorted(glob.glob(os.path.join(PKG, "lipasr", "*.py")) + glob.glob(os.path.join(PKG, "csrc", "*")))


def test_every_variable_named_in_the_sources_is_a_row():
    assert len(NAMES) == len(knobs.TABLE)
    found = {}
    for path in _sources():
        for name in re.findall(r"""["'](LIPASR_[A-Z0-9_]+)["']""", open(path, errors="replace").read()):
            found.setdefault(name, os.path.basename(path))
    assert found and not {n: f for n, f in found.items() if n not in NAMES}
    # the rows the package itself reads are all in use
    assert {row.name for row in knobs.TABLE if row.reader in ("lipasr", "native")} <= set(found)


def test_only_knobs_reads_the_environment_for_them():
    for path in glob.glob(os.path.join(PKG, "lipasr", "*.py")):
        if os.path.basename(path) == "knobs.py":
            continue
        text = open(path).read()
        for m in re.finditer(r"\benviron\b|getenv", text):  # (parallel.py reads torch.distributed's own variables)
            line = text[text.rfind("\n", 0, m.start()) + 1:text.find("\n", m.end())]
            assert "LIPASR_" not in line, (path, line)


def test_get_reads_at_call_time_and_parses_as_the_table_says(monkeypatch):
    for row in knobs.TABLE:
        monkeypatch.delenv(row.name, raising=False)
        assert knobs.get(row.name) == row.default
    monkeypatch.setenv("LIPASR_FLAG_TIMEOUT_MS", "40")
    monkeypatch.setenv("LIPASR_GPU_FLAGS", "0")
    assert knobs.get("LIPASR_FLAG_TIMEOUT_MS") == 40 and knobs.get("LIPASR_GPU_FLAGS") == "0"
    monkeypatch.setenv("LIPASR_FLAG_TIMEOUT_MS", "soon")
    with pytest.raises(ValueError):
        knobs.get("LIPASR_FLAG_TIMEOUT_MS")
    with pytest.raises(KeyError):
        knobs.get("LIPASR_NO_SUCH_KNOB")


def test_readme_lists_the_table():
    text = open(os.path.join(ROOT, "README.md")).read()
    section = text[text.index("## Environment variables"):]
    section = section[:section.index("\n## ", 1)] if "\n## " in section[1:] else section
    rows = re.findall(r"^\| `(LIPASR_[A-Z0-9_]+)` \| ([^|]*) \| ([^|]*) \|", section, flags=re.M)
    assert [r[0] for r in rows] == [row.name for row in knobs.TABLE]
    for (name, default, kind), row in zip(rows, knobs.TABLE):
        assert default.strip() == ("(unset)" if row.default in (None, "") else f"`{row.default}`"), name
        assert kind.strip() == row.kind + ("" if row.reader == "lipasr" else ", " + row.reader), name
