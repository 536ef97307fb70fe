"""Compare two `bench.py --dump-outputs` directories array by array (no GPU).

    python tools/cmp_dumps.py PARENT_DIR NEW_DIR [OUT_TXT]

Per array: bit-equal or not; for the others the largest |a - b| relative to the largest |a| of the array, and the
error norm relative to the array's norm.
"""
import os
import sys

import numpy as np


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    names = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
    missing = [f for f in names if not os.path.exists(os.path.join(b_dir, f))]
    lines, differ = [], 0
    for f in names:
        if f in missing:
            continue
        a, b = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        if a.shape == b.shape and a.tobytes() == b.tobytes():
            lines.append(f"{f[:-4]:40s} bit-equal")
            continue
        differ += 1
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        mx = np.abs(a64 - b64).max() / max(np.abs(a64).max(), 1e-300)
        nr = np.linalg.norm((a64 - b64).ravel()) / max(np.linalg.norm(a64.ravel()), 1e-300)
        lines.append(f"{f[:-4]:40s} differs: max |a - b| / max |a| = {mx:.3e}, |a - b| / |a| = {nr:.3e}")
    head = f"{len(names) - len(missing)} arrays compared, {differ} differ" + (f", missing in new: {missing}" if missing else "")
    text = "\n".join([head] + lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text)


if __name__ == "__main__":
    main()
