"""What the kernel-pick tables (gemm_picks.py, attn_picks.py) share: asking a probe under an environment in a fresh process (the dispatch switches are read once, when the
library loads), and the table format — the distinct picks once, then per environment one 16-bit index per row, deflated and base64-coded (environments and rows repeat
themselves enough to shrink hundreds of KB of digits to tens); each tool's `--show` prints its table row by row."""
import array
import base64
import hashlib
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def env_key(env):
    return ",".join(f"{k}={v}" for k, v in sorted(env.items())) or "default"


def rows_digest(rows):
    return hashlib.sha256("\n".join(" ".join(map(str, r)) for r in rows).encode()).hexdigest()


def load_lib():
    sys.path.insert(0, ROOT)
    import ldx_amd
    return ldx_amd.lib.load()


def picks_of_env(script, env):
    """The picks `script --dump` prints with only `env` of the LDX_* switches set."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("LDX_")}
    r = subprocess.run([sys.executable, os.path.abspath(script), "--dump"], env=dict(clean, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return [tuple(p) for p in json.loads(r.stdout)]


def encode(per_env):
    uniq = sorted({p for picks in per_env.values() for p in picks})
    idx = {p: i for i, p in enumerate(uniq)}
    return uniq, {k: base64.b64encode(zlib.compress(array.array("H", [idx[p] for p in picks]).tobytes(), 9)).decode() for k, picks in per_env.items()}


def decode(table, key):
    a = array.array("H")
    a.frombytes(zlib.decompress(base64.b64decode(table["envs"][key])))
    return [tuple(table["picks"][i]) for i in a]


def load_table(path):
    with open(path) as f:
        return json.load(f)


def write_table(path, per_env, rows, **header):
    """header: what the tool wants kept beside the picks (field and family names)."""
    uniq, envs = encode(per_env)
    t = dict(header, n_rows=len(rows), rows_sha256=rows_digest(rows), picks=[list(p) for p in uniq], envs=envs)
    with open(path, "w") as f:          # one key per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(t[k], sort_keys=True, separators=(',', ':'))}" for k in sorted(t)) + "\n}\n")
    return t


# ---- a table of (count, 32-bit digest) per row, where every row of every environment is its own pick (tests/tools/plan_trace.py): per environment the counts as
# 16-bit values, deflated, and the digests as 4 bytes each, base64-coded
def encode_digests(picks):
    return {"records": base64.b64encode(zlib.compress(array.array("H", [p[0] for p in picks]).tobytes(), 9)).decode(),
            "digests": base64.b64encode(bytes.fromhex("".join(p[1] for p in picks))).decode()}


def decode_digests(table, key):
    e = table["envs"][key]
    n = array.array("H")
    n.frombytes(zlib.decompress(base64.b64decode(e["records"])))
    d = base64.b64decode(e["digests"])
    return [(c, d[4 * i:4 * i + 4].hex()) for i, c in enumerate(n)]


def write_digest_table(path, per_env, rows, **header):
    t = dict(header, n_rows=len(rows), rows_sha256=rows_digest(rows), envs={k: encode_digests(p) for k, p in per_env.items()})
    with open(path, "w") as f:          # one key per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(t[k], sort_keys=True, separators=(',', ':'))}" for k in sorted(t)) + "\n}\n")
    return t


def cli(tool):
    """The command line of a pick tool: a module with all_rows, ENVS, TABLE, picks_of_current_env, load_table, write_table and describe (usage: its docstring);
    optional: decode (its own table format), picks_of_envs (its environments several at a time), mismatch (more to say about a row that differs)."""
    rows, dec = tool.all_rows(), getattr(tool, "decode", decode)
    if "--rows" in sys.argv:
        print("\n".join(" ".join(map(str, r)) for r in rows))
    elif "--show" in sys.argv:
        t = tool.load_table()
        for k in t["envs"]:
            for r, p in zip(rows, dec(t, k)):
                print(k, tool.describe(r, p))
    elif "--dump" in sys.argv:
        print(json.dumps(tool.picks_of_current_env(rows)))
    else:
        per_env = tool.picks_of_envs(tool.ENVS) if hasattr(tool, "picks_of_envs") else {env_key(e): picks_of_env(tool.__file__, e) for e in tool.ENVS}
        if "--write" in sys.argv:
            tool.write_table(per_env, rows)
            print(f"wrote {len(rows)} rows x {len(tool.ENVS)} environments to {tool.TABLE}")
            return
        t = tool.load_table()
        for e in tool.ENVS:          # what differs between the current build's picks and the table
            k, picks = env_key(e), per_env[env_key(e)]
            old = dec(t, k) if k in t["envs"] else []
            moved = [i for i in range(len(rows)) if i >= len(old) or old[i] != picks[i]]
            print(f"{k}: {len(rows)} rows, {len(moved)} differ from the table")
            for i in moved[:20]:
                print("   ", tool.describe(rows[i], picks[i]), " (table:", old[i] if i < len(old) else None, ")")
            if moved and hasattr(tool, "mismatch") and moved[0] < len(old):
                print("   ", tool.mismatch(e, moved[0], rows[moved[0]], picks[moved[0]], old[moved[0]]))
