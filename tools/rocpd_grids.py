#!/usr/bin/env python3
"""Launches grouped by kernel AND grid from a rocprofv3 rocpd result (…_results.db):  python tools/rocpd_grids.py <db> [name substring ...]
(default substrings: the BatchNorm and zero-fill kernels).  One line per (kernel, grid): threads, workgroups, calls, avg / min us."""
import sqlite3
import sys


def _one(names, what, pick):
    found = [n for n in names if pick(n)]
    if len(found) != 1:
        sys.exit(f'rocpd_grids: expected exactly one {what}, found {found or "none"} among {sorted(names)} (the rocpd schema changed?)')
    return found[0]


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    db = sqlite3.connect(sys.argv[1])
    subs = sys.argv[2:] or ['bn_reduce', 'bn_apply', 'bn_bwd_apply', 'zero_many']
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    disp = _one(tabs, 'kernel dispatch table', lambda t: t.startswith('rocpd_kernel_dispatch'))
    sym = _one(tabs, 'kernel symbol table', lambda t: t.startswith('rocpd_info_kernel_symbol'))
    cols = [r[1] for r in db.execute(f'pragma table_info({disp})')]
    grid = _one(cols, 'grid size x column', lambda c: 'grid' in c.lower() and c.lower().endswith('x'))
    wg = _one(cols, 'workgroup size x column', lambda c: 'workgroup' in c.lower() and c.lower().endswith('x'))
    rows = db.execute(f'select s.display_name, d.{grid}, d.{wg}, count(*), avg(d.end - d.start), min(d.end - d.start) from {disp} d join {sym} s '
                      f'on d.kernel_id = s.id group by s.display_name, d.{grid} order by 5 desc').fetchall()
    print('kernel | grid (threads) | workgroups | calls | avg us | min us')
    for name, g, w, n, avg, mn in rows:
        if any(s in name for s in subs):
            print('%s | %d | %d | %d | %.1f | %.1f' % (name[:70], g, g // max(w, 1), n, avg / 1e3, mn / 1e3))


if __name__ == '__main__':
    main()
