"""Lifecycle of every handle from plain C++ (tests/emu/lifecycle_main.cpp): create, grow, update,
solve and destroy in both orders, through the C ABI only, linked against the emulator library.
Here the program's own status checks are the test; its header comment has the recipe of the
sanitizer run it was written for (there, a buffer a handle does not free is a leak report)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lifecycle_program(tmp_path):
    from runlmc_amd.build import EMU_DIR, build_emu
    lib = build_emu()
    gxx = shutil.which('g++')
    assert gxx, 'g++ not found'
    exe = str(tmp_path / 'lifecycle')
    name = os.path.basename(lib)[3:-3]
    subprocess.check_call([gxx, '-std=c++17', '-O1', '-Wall', '-I' + os.path.join(ROOT, 'include'),
                           os.path.join(EMU_DIR, 'lifecycle_main.cpp'), '-o', exe, '-L' + EMU_DIR,
                           '-l' + name, '-Wl,-rpath,' + EMU_DIR, '-pthread'])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert 'lifecycle ok (emu-host)' in out.stdout
