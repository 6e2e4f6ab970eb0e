#!/usr/bin/env python3
"""tools/far_ab_hash.py: sha256 of the result bytes (bp1, bp2, up1, up2, hp, logZ of every pair) of the three CONTRAfold batches of
tests/test_gpu_far_wave.py, plain and under RH_FAR2=1, computed by the library of the tree this file lies in.  Run it in two trees
(two builds) on one machine and compare the lines: the block products promise the same bits, so any difference is a bug.
Extra switches: NAME=VALUE arguments, e.g. RH_FAR_WAVE=0."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import ractip_amd
    from test_gpu_far_wave import KEYS, batches
    extra = dict(a.split("=", 1) for a in sys.argv[1:])
    b = batches()
    for far2 in (None, "1"):
        env = dict(extra)
        if far2:
            env["RH_FAR2"] = far2
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            c = ractip_amd.Context(device=0)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        try:
            for name in (1, 2, 3):
                c.batch_upload(b[name])
                c.batch_compute()
                h = hashlib.sha256()
                for p in range(len(b[name])):
                    r = c.batch_results(p)
                    for key in KEYS:
                        h.update(r[key].tobytes())
                print("batch %d %-12s %s  %s" % (name, " ".join("%s=%s" % kv for kv in sorted(env.items())) or "default", h.hexdigest(),
                                                 " ".join(k[1] for k in c.batch_kernels()[:2])), flush=True)
        finally:
            c.close()


if __name__ == "__main__":
    main()
