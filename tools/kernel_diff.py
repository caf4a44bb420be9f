"""Compare the gfx950 instructions of kernels between two builds of one object file, e.g. to show that an instance a change
should not touch still compiles to the same code:

    python tools/kernel_diff.py OLD.o NEW.o [old_name=new_name ...]

Kernels are matched by (mangled) name; `old=new` pairs match kernels that were renamed (a kernel that became a template
instance).  Addresses, encodings and the padding behind a kernel's last instruction are ignored; everything else --
opcode, registers, immediates, order -- counts.  Needs only the ROCm LLVM tools, no GPU."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
PAD = ('s_nop 0', '...', 's_code_end')


def kernels(obj, arch='gfx950'):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, 'fat.bin'), os.path.join(d, 'dev.co')
        subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', obj, fat])
        subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + fat,
                               '--targets=hipv4-amdgcn-amd-amdhsa--' + arch, '--output=' + co])
        text = subprocess.check_output([os.path.join(LLVM, 'llvm-objdump'), '-d', co], text=True)
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(\S+)>:', line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        t = line.split('//')[0].strip()
        if cur is None or not t:
            continue
        cur.append(re.sub(r'<[^>+]+(\+0x[0-9a-f]+)?>', lambda mm: '<K' + (mm.group(1) or '') + '>', t))
    for body in out.values():
        while body and body[-1] in PAD:
            body.pop()
    return out


def main(argv):
    old, new = kernels(argv[1]), kernels(argv[2])
    renamed = dict(a.split('=') for a in argv[3:])
    same = True
    for name, body in old.items():
        other = new.get(renamed.get(name, name))
        if other is None:
            print('%-70s %6d  missing in the new build' % (name[:70], len(body)))
            same = False
            continue
        if body == other:
            print('%-70s %6d  identical' % (name[:70], len(body)))
            continue
        same = False
        diff = [l for l in difflib.unified_diff(body, other, lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
        print('%-70s %6d -> %d  DIFFERS in %d lines' % (name[:70], len(body), len(other), len(diff)))
        for l in diff[:40]:
            print('    ' + l)
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv))
