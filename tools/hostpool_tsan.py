"""ThreadSanitizer stress of the host thread pool of the narrowed upload (HostPool, csrc/transform.hip): the class is cut out of the
source verbatim, four caller threads run 20 000 short jobs each with task counts around the worker count, every task must run
exactly once, TSan must stay silent.  CPU only.    python tools/hostpool_tsan.py"""
import ctypes, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
s = open(os.path.join(ROOT, "rankcompv3.jl_amd", "csrc", "transform.hip")).read()
a = s.index("class HostPool {"); b = s.index("};", s.index("    uint64_t gen_ = 0;", a)) + 2
src = '''#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
''' + s[a:b] + '''
int main()
{
    std::atomic<long> bad{0};
    std::vector<std::thread> callers;
    for (int c = 0; c < 4; ++c)
        callers.emplace_back([&, c] {
            for (int rep = 0; rep < 20000; ++rep) {
                const int n = 1 + (rep * 7 + c) % 13;
                std::vector<int> hits(n, 0);
                HostPool::get(2 + rep % 7).run(n, [&](int t) { hits[t]++; });
                for (int t = 0; t < n; ++t) if (hits[t] != 1) bad++;
            }
        });
    for (auto &t : callers) t.join();
    printf("HostPool stress: %ld tasks ran a number of times other than once\\n", bad.load());
    return bad.load() != 0;
}
'''


def no_aslr():
    """ThreadSanitizer (GCC 11's libtsan) puts its shadow memory at fixed addresses and aborts with "unexpected memory mapping"
    when a kernel with more mmap randomisation (vm.mmap_rnd_bits = 32) loads the binary outside the ranges it knows; newer
    runtimes re-exec themselves without randomisation.  This does that for the child alone (personality flag ADDR_NO_RANDOMIZE)."""
    libc = ctypes.CDLL(None)
    libc.personality(libc.personality(0xFFFFFFFF) | 0x0040000)


with tempfile.TemporaryDirectory() as tmp:   # a directory of its own: a fixed name in a shared /tmp may belong to another user
    cpp = os.path.join(tmp, "hostpool_stress.cpp")
    open(cpp, "w").write(src)
    for flags, name in ((["-O1", "-g", "-fsanitize=thread"], "tsan"), (["-O2"], "plain")):
        exe = os.path.join(tmp, "hostpool_" + name)
        subprocess.check_call(["g++", *flags, "-pthread", "-o", exe, cpp])
        out = subprocess.run([exe], capture_output=True, text=True, preexec_fn=no_aslr)
        print(name + ":", out.stdout.strip(), "| stderr lines:", len(out.stderr.strip().splitlines()), "| exit", out.returncode)
        if out.returncode or out.stderr.strip():
            print(out.stderr[:4000]); sys.exit(1)
print("hostpool_tsan: clean")
