"""CPU: the hidden kernel arguments of every kernel the AQL path dispatches (fql_amd/csrc/fql_aql.h).

Stream-less updates run as pre-built AQL packets, and AqlRuntime::fill_kernarg writes their kernarg blocks itself: the explicit
arguments, then of the code-object-v5 hidden block only the block counts (+0), the group sizes (+12) and the grid dimensions (+64),
at align8(end of the explicit arguments).  Every other hidden argument stays zero.  That is right for remainders (the grids are
uniform) and global offsets (there are none), and wrong for anything else: a device printf or assert adds hidden_hostcall_buffer,
which would be a null pointer on the AQL path, and other hidden arguments (heap, queue, dynamic LDS size, ...) would read zero.

The gfx950 code object is read the way the engine reads it (the .hip_fatbin section of libfql_amd.so, the amdgcn gfx950 entry of the
clang offload bundle), and its AMDGPU metadata note is decoded with msgpack."""
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = 'gfx950'

# what fill_kernarg writes, or correctly leaves at zero
ALLOWED_HIDDEN = {f'hidden_{k}_{a}' for k in ('block_count', 'group_size', 'remainder', 'global_offset') for a in 'xyz'} | {'hidden_grid_dims'}
# offsets fill_kernarg hard-codes, relative to align8(end of the explicit arguments)
FIXED_OFFSETS = {'hidden_block_count_x': 0, 'hidden_group_size_x': 12, 'hidden_grid_dims': 64}
NT_AMDGPU_METADATA = 32


def _sections(elf):
    """{name: bytes} of an ELF64 little-endian image."""
    assert elf[:4] == b'\x7fELF' and elf[4] == 2 and elf[5] == 1, 'not an ELF64 little-endian image'
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from('<HHH', elf, 0x3A)
    hdrs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + i * shentsize) for i in range(shnum)]
    _, _, _, _, stro, strsz, _, _, _, _ = hdrs[shstrndx]
    names = elf[stro:stro + strsz]
    out = {}
    for name, typ, _, _, off, size, _, _, _, _ in hdrs:
        nm = names[name:names.index(b'\0', name)].decode()
        out[nm] = (typ, elf[off:off + size] if typ != 8 else b'')   # SHT_NOBITS has no file contents
    return out


def code_object_from_library(path, isa=ISA):
    """AqlRuntime::read_code_object: the `isa` entry of the uncompressed clang offload bundle in .hip_fatbin."""
    with open(path, 'rb') as f:
        secs = _sections(f.read())
    assert '.hip_fatbin' in secs, f'{path} has no .hip_fatbin section'
    fb = secs['.hip_fatbin'][1]
    assert fb[:24] == b'__CLANG_OFFLOAD_BUNDLE__', '.hip_fatbin is not an uncompressed offload bundle (the AQL path cannot read it either)'
    n, = struct.unpack_from('<Q', fb, 24)
    o = 32
    for _ in range(n):
        off, size, tl = struct.unpack_from('<QQQ', fb, o)
        triple = fb[o + 24:o + 24 + tl].decode()
        o += 24 + tl
        if 'amdgcn' in triple and isa in triple and size > 0:
            return fb[off:off + size]
    raise AssertionError(f'no {isa} code object in the bundle of {path}')


def kernel_metadata(code_object):
    """The amdhsa.kernels list of the NT_AMDGPU_METADATA note (msgpack)."""
    msgpack = pytest.importorskip('msgpack')
    for typ, data in _sections(code_object).values():
        if typ != 7:   # SHT_NOTE
            continue
        o = 0
        while o + 12 <= len(data):
            namesz, descsz, ntype = struct.unpack_from('<III', data, o)
            name = data[o + 12:o + 12 + namesz].rstrip(b'\0')
            d0 = o + 12 + ((namesz + 3) & ~3)
            if name == b'AMDGPU' and ntype == NT_AMDGPU_METADATA:
                return msgpack.unpackb(data[d0:d0 + descsz], raw=False)['amdhsa.kernels']
            o = d0 + ((descsz + 3) & ~3)
    raise AssertionError('no AMDGPU metadata note in the code object')


def layout_problems(kernel):
    """What fill_kernarg would get wrong for this kernel (empty: nothing)."""
    args = kernel.get('.args', [])
    explicit = [a for a in args if not a['.value_kind'].startswith('hidden_')]
    hidden = {a['.value_kind']: a for a in args if a['.value_kind'].startswith('hidden_')}
    hb = (max((a['.offset'] + a['.size'] for a in explicit), default=0) + 7) & ~7
    out = []
    extra = sorted(set(hidden) - ALLOWED_HIDDEN)
    if extra:
        out.append(f'hidden arguments fill_kernarg leaves at zero: {extra}')
    for kind, rel in FIXED_OFFSETS.items():
        if kind in hidden and hidden[kind]['.offset'] != hb + rel:
            out.append(f'{kind} at offset {hidden[kind][".offset"]}, fill_kernarg writes it at {hb + rel}')
    if hidden and kernel['.kernarg_segment_size'] < hb + 72:
        out.append(f'kernarg segment of {kernel[".kernarg_segment_size"]} bytes: fill_kernarg only writes the hidden block from {hb + 72}')
    return out


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_every_kernel_has_only_the_hidden_arguments_fill_kernarg_writes(lib):
    from fql_amd import _cabi
    kernels = kernel_metadata(code_object_from_library(_cabi.LIB_PATH))
    assert len(kernels) >= 20
    with_hidden = [k for k in kernels if any(a['.value_kind'].startswith('hidden_') for a in k.get('.args', []))]
    assert with_hidden, 'no kernel reads blockDim / gridDim: the offset checks below would check nothing'
    bad = {k['.name']: p for k in kernels for p in [layout_problems(k)] if p}
    assert not bad, ('kernels whose kernarg layout the AQL path (fql_aql.h, AqlRuntime::fill_kernarg) does not fill: '
                     f'{bad}.  Remove the device printf / assert, or debug that kernel with FQL_NO_GRAPH=1 or on a caller\'s stream '
                     '(the captured graph, which HIP fills), or extend fill_kernarg to write these arguments.')


SELF_CHECK_SRC = r'''
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void plain_kernel(float* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= 2.0f;
}
__global__ void printing_kernel(float* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) printf("n %d x0 %f\n", n, x[0]);
}
'''


def test_layout_check_flags_a_kernel_with_printf(tmp_path):
    """The check above bites: of two kernels compiled here, the one that calls printf is flagged, the one that only reads
    blockDim is not."""
    hipcc = shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)
    if hipcc is None:
        pytest.skip('hipcc not found')
    src, co = tmp_path / 'k.hip', tmp_path / 'k.co'
    src.write_text(SELF_CHECK_SRC)
    subprocess.run([hipcc, '-O3', f'--offload-arch={ISA}', '--cuda-device-only', '--no-gpu-bundle-output', '-c', '-o', str(co), str(src)],
                   check=True, capture_output=True, timeout=300)
    kernels = {k['.name']: k for k in kernel_metadata(co.read_bytes())}
    plain = next(v for n, v in kernels.items() if 'plain_kernel' in n)
    printing = next(v for n, v in kernels.items() if 'printing_kernel' in n)
    assert any(a['.value_kind'] == 'hidden_block_count_x' for a in plain['.args'])
    assert layout_problems(plain) == []
    problems = layout_problems(printing)
    assert problems and 'hidden_hostcall_buffer' in problems[0], problems
