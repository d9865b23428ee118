"""The -DLDPC_EXPERIMENTS build of the library, which __graft_entry__.build() makes beside the product as
ldpc_toolbox_amd/lib/libldpc_toolbox_exp.so.  It carries the opt-in forms the product left behind in round 5 -- the
slice-persistent layered kernel and continuous batching.  Their tests are decorated with `on_experiments_build`: in a
process that loaded the experiments build they run as they are; in one that loaded the product (one process holds one
HIP library) the same test runs in a child pytest process whose LDPC_TOOLBOX_LIB selects the experiments build, and it
passes only if it passed there."""
import functools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP_LIB = os.path.join(ROOT, "ldpc_toolbox_amd", "lib", "libldpc_toolbox_exp.so")


def experiments_build():
    """True when the loaded library was built with -DLDPC_EXPERIMENTS"""
    import ldpc_toolbox_amd as lt
    from frames import alist
    return lt.LdpcDecoder(alist("ar4ja:1/2:1024"), "Minsumf32").get("experiments") == 1


def on_experiments_build(test):
    @functools.wraps(test)
    def run(*args, **kwargs):
        if experiments_build():
            return test(*args, **kwargs)
        assert os.path.exists(EXP_LIB), f"{EXP_LIB} is missing: __graft_entry__.build() makes it"
        # this test's node (its parameters included) by the absolute path of its module, whatever pytest's rootdir
        name = os.environ["PYTEST_CURRENT_TEST"].rsplit(" (", 1)[0].split("::", 1)[1]
        node = os.path.abspath(test.__code__.co_filename) + "::" + name
        env = dict(os.environ, LDPC_TOOLBOX_LIB=EXP_LIB)
        env.pop("PYTEST_CURRENT_TEST", None)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rs", "-p", "no:cacheprovider", node],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0 and "1 passed" in r.stdout, (r.stdout[-3000:], r.stderr[-2000:])
    return run
