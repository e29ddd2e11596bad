"""Every LDX_* environment switch of the native library is read in one file, csrc/ldx_switches.cpp ("Picks and switches"): a plain text scan over the
native sources, no build and no GPU.  getenv occurs in that file only, and every quoted "LDX_..." name occurs there once and in no other native source.  One
name is read into two fields with two defaults (LDX_ATTN_PIPE_MINWG: 256 for D = 40, 192 for D = 128) and so occurs twice.  (tests/tools/hip_standin.cpp and its
LDX_STANDIN_* names are not part of the library.)"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lightdiffusion-next_amd", "csrc")
SWITCHES = "ldx_switches.cpp"
NAME = re.compile(r'"(LDX_[A-Z0-9_]+)"')
TWICE = {"LDX_ATTN_PIPE_MINWG"}


def sources():
    out = {}
    for ext in ("hip", "cpp", "h", "inc"):
        for path in glob.glob(os.path.join(CSRC, "*." + ext)):
            with open(path, encoding="utf-8") as f:
                out[os.path.basename(path)] = f.read()
    assert SWITCHES in out and len(out) > 40, sorted(out)
    return out


def test_getenv_only_in_the_switches_source():
    assert [name for name, text in sorted(sources().items()) if "getenv" in text] == [SWITCHES]


def test_every_switch_name_once_and_only_in_the_switches_source():
    src = sources()
    elsewhere = {name: sorted(set(NAME.findall(text))) for name, text in src.items() if name != SWITCHES and NAME.search(text)}
    assert elsewhere == {}
    names = NAME.findall(src[SWITCHES])
    print(len(set(names)), "switches:", " ".join(sorted(set(names))))
    assert {n: names.count(n) for n in set(names) if names.count(n) != (2 if n in TWICE else 1)} == {}
