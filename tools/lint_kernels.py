"""Compile every csrc/*.hip to gfx950 assembly and list each kernel's registers, spills, scratch and LDS bytes.
Scratch (private segment) > 0 in a hot kernel is almost always an accident: an array indexed with a runtime value
(the AWQ clip search ran 3x slower that way). No GPU needed.   python tools/lint_kernels.py [file.hip ...]

--against <other csrc directory> compiles the same files of another tree (a checkout of the parent commit, say) as well and
prints, per kernel, both sides' columns and `same` or `differs` for its instruction stream and kernel descriptor; what a file's
assembly holds outside its kernels (device functions, data, metadata) is one more row per file. Only the `__hip_cuid_*` symbol
and the numbering of local labels are normalised. This is the "identical device code" check of a refactor (profiles/NOTES.md)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from llmc_amd.build import CSRC, FILE_FLAGS, FLAGS, HIPCC  # noqa: E402

KEYS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
        'group_segment_fixed_size')
HEAD = ('vgpr', 'agpr', 'sgpr', 'vspill', 'sspill', 'scratch', 'lds')
FMT = ' '.join('{:>7s}' for _ in KEYS)


def assembly(csrc, src):
    """Device assembly of csrc/src with the build's flags, or (None, error). Compiled from inside csrc with relative paths, so
    that two trees give the same text wherever they lie."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'k.s')
        cmd = [HIPCC] + FLAGS + FILE_FLAGS.get(src, []) + ['-I../../include', '-I.', '-S', '--cuda-device-only', '-o', out, src]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=csrc)
        if r.returncode != 0:
            return None, r.stderr[-400:]
        return open(out).read(), ''


def short_name(name):
    dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    return re.sub(r'\(.*', '', (dem or name).replace('(anonymous namespace)::', ''))[:64]


def metadata(txt):
    """{mangled kernel name: tuple of KEYS' values} from the assembly's amdhsa.kernels metadata, in file order."""
    rows = {}
    for blk in txt.split('  - .agpr_count:')[1:]:
        blk = '.agpr_count:' + blk
        def f(key):
            m = re.search(r'\.' + key + r':\s+(\S+)', blk)
            return m.group(1) if m else '?'
        rows[f('name')] = tuple(f(k) for k in KEYS)
    return rows


def split_kernels(txt, names):
    """{name: normalised text of the kernel's function body and .amdhsa_kernel block}, plus '' -> everything else."""
    txt = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', txt)
    parts = {}
    for n in names:
        body = re.search(r'^' + re.escape(n) + r':.*?^\.Lfunc_end\d+:\n', txt, re.S | re.M)
        desc = re.search(r'^\s*\.amdhsa_kernel ' + re.escape(n) + r'\n.*?\.end_amdhsa_kernel\n', txt, re.S | re.M)
        got = ''
        for m in sorted((m for m in (body, desc) if m), key=lambda m: -m.start()):      # cut from the back: offsets stay valid
            got = txt[m.start():m.end()] + got
            txt = txt[:m.start()] + txt[m.end():]
        parts[n] = got
    parts[''] = txt
    for n, t in parts.items():
        labels = {}
        parts[n] = re.sub(r'\.L(?:BB|func_end|func_begin|tmp|JTI)\d+(?:_\d+)*',
                          lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), t)
    return parts


def lint_one(src):
    txt, err = assembly(CSRC, src)
    return src, None if txt is None else [(short_name(n), v) for n, v in metadata(txt).items()], err


def against_one(other, src):
    ours, err = assembly(CSRC, src)
    if ours is None:
        return src, None, 'this tree: ' + err
    if not os.path.exists(os.path.join(other, src)):
        return src, None, 'not in ' + other
    theirs, err = assembly(other, src)
    if theirs is None:
        return src, None, 'other tree: ' + err
    mo, mt = metadata(ours), metadata(theirs)
    names = list(mo) + [n for n in mt if n not in mo]
    po, pt = split_kernels(ours, names), split_kernels(theirs, names)
    rows = [(short_name(n), mo.get(n), mt.get(n), n in mo and n in mt and po[n] == pt[n] and mo[n] == mt[n]) for n in names]
    rows.append(('(outside the kernels)', None, None, po[''] == pt['']))
    return src, rows, ''


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('files', nargs='*', help='csrc/*.hip file names (default: all)')
    ap.add_argument('--against', metavar='CSRC_DIR', help="another tree's csrc directory to compare the device code with")
    args = ap.parse_args()
    files = args.files or sorted(f for f in os.listdir(CSRC) if f.endswith('.hip'))
    other = os.path.abspath(args.against) if args.against else None
    with ThreadPoolExecutor(8) as ex:
        res = list(ex.map((lambda s: against_one(other, s)) if other else lint_one, files))
    cols = FMT.format(*HEAD)
    print(f'{"kernel":64s} {cols}' + (f' | {cols}  code' if other else ''))
    bad = kernels = differs = 0
    for src, rows, err in res:
        print(f'-- {src}')
        if rows is None:
            print('   compile failed:', err)
            bad += 1
            continue
        for row in rows:
            if not other:
                n, v = row
                flag = '  <-- scratch' if v[5] not in ('0', '?') else ''
                print(f'{n:64s} {FMT.format(*v)}{flag}')
                continue
            n, v, t, same = row
            blank = ('',) * len(KEYS)
            kernels += v is not None or t is not None
            differs += not same
            print(f'{n:64s} {FMT.format(*(v or blank))} | {FMT.format(*(t or blank))}  {"same" if same else "differs"}')
    if other:
        print(f'{kernels} kernels of {len(res) - bad} files compared with {other}: {differs} rows differ, {bad} files failed to compile')
    return 1 if bad or differs else 0


if __name__ == '__main__':
    sys.exit(main())
