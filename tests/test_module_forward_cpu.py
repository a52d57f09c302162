"""CPU: fql_module_forward (agent.network.select(name)(...)) is declared in include/fql_amd.h, exported by libfql_amd.so and bound in
fql_amd/_cabi.py; a NULL handle is FQL_E_INVALID; the host mirror names each kind's modules.  Nothing here launches GPU compute."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from fql_amd import _cabi
    return _cabi.load()


def test_module_forward_is_declared_exported_and_bound(lib):
    from fql_amd import _cabi
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'fql_amd.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+fql_module_forward\s*\(([^)]*)\)', src)
    assert m, 'fql_module_forward is not declared in include/fql_amd.h'
    assert len(m.group(1).split(',')) == 8        # h, module, observations, actions, times, n, out, stream
    assert hasattr(lib, 'fql_module_forward')
    res, args = _cabi.SYMBOLS['fql_module_forward']
    assert len(args) == 8
    assert lib.fql_module_forward.argtypes == args and lib.fql_module_forward.restype is res


def test_null_handle_is_invalid(lib):
    from fql_amd import _cabi
    assert lib.fql_module_forward(None, b'critic', None, None, None, 1, None, None) == _cabi.FQL_E_INVALID


def test_abi_version_is_unchanged(lib):
    assert lib.fql_abi_version() == 1


def test_mirror_module_tables():
    """The kinds' modules as the issue's table has them; BC and CFGRL have none."""
    import fql_amd
    from fql_amd import bc, cfgrl, iql_diffusion
    pair = {'critic', 'target_critic'}
    assert set(fql_amd.FQLAgent._modules) == pair | {'actor_bc_flow', 'actor_onestep_flow'}
    assert set(fql_amd.IFQLAgent._modules) == pair | {'value', 'actor_flow'}
    assert set(fql_amd.ReBRACAgent._modules) == pair and set(fql_amd.SACAgent._modules) == pair
    assert set(fql_amd.IQLAgent._modules) == pair | {'value'}
    assert set(iql_diffusion.IQLDiffusionAgent._modules) == pair | {'value'}
    assert not bc.BCAgent._modules and not cfgrl.CFGRLAgent._modules
