"""Device assembly of every csrc/*.hip file in two trees, compared: the proof that a source refactor moved no instruction.

    python profiles/compare_device_asm.py OLD [NEW]

OLD / NEW: a checkout's root directory or a git revision of this repository; NEW defaults to the working tree.  Each file is
compiled with exactly the flags its own tree's build.py gives it plus `--offload-device-only -S` (hipcc only, no GPU), the
`.ident` line is dropped, and the files whose assembly differs are printed.  Both trees are staged in turn at the SAME
temporary path: the assembly holds no source path, but hipcc names one symbol (__hip_cuid_<hash>) after a hash of it.
Exit status 1 when any file differs or exists on one side only.
"""
import concurrent.futures
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'occlusions-4d_amd'


def stage(spec, dst):
    """csrc/, build.py and include/ of a checkout or a revision at dst."""
    if os.path.isdir(os.path.join(spec, PKG)):
        shutil.copytree(os.path.join(spec, PKG, 'csrc'), os.path.join(dst, PKG, 'csrc'))
        shutil.copy(os.path.join(spec, PKG, 'build.py'), os.path.join(dst, PKG))
        shutil.copytree(os.path.join(spec, 'include'), os.path.join(dst, 'include'))
    else:
        tar = subprocess.run(['git', '-C', ROOT, 'archive', spec, PKG + '/csrc', PKG + '/build.py', 'include'], check=True,
                             stdout=subprocess.PIPE).stdout
        os.makedirs(dst)
        subprocess.run(['tar', '-x', '-C', dst], input=tar, check=True)


def assembly(spec, tmp):
    root = os.path.join(tmp, 'tree')
    stage(spec, root)
    mod = importlib.util.spec_from_file_location('occ4d_build', os.path.join(root, PKG, 'build.py'))
    b = importlib.util.module_from_spec(mod)
    mod.loader.exec_module(b)

    def one(src):
        cmd = [b._hipcc()] + b.FLAGS + b.FILE_FLAGS.get(src, []) + ['--offload-device-only', '-S', os.path.join(b.CSRC, src), '-o', '-']
        text = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout.decode()
        return src, [l for l in text.splitlines() if not l.lstrip().startswith('.ident')]

    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        out = dict(ex.map(one, b.sources()))
    shutil.rmtree(root)
    return out


def main(argv):
    if not 1 <= len(argv) <= 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        old = assembly(argv[0], tmp)
        new = assembly(argv[1] if len(argv) > 1 else ROOT, tmp)
    names = sorted(set(old) | set(new))
    differ = [f for f in names if old.get(f) != new.get(f)]
    for f in names:
        print('%-24s %6d lines  %s' % (f, len(new.get(f, old.get(f))), 'DIFFERS' if f in differ else 'identical'))
    print('%d of %d files differ%s' % (len(differ), len(names), ': ' + ' '.join(differ) if differ else ''))
    return 1 if differ else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
