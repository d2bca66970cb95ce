"""First rows of restarted episodes (mate_engine_enable_first_rows), the parts that need no GPU: the built library exports the entry
point, the binding declares it and its struct, and the Python surface takes the keywords with the feature off by default."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_point_and_python_takes_the_keywords():
    from mate_amd import _native
    assert os.path.exists(_native.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, 'mate_engine_enable_first_rows')
    assert 'mate_engine_enable_first_rows' in _native.EXPORTED_SYMBOLS
    with open(os.path.join(ROOT, 'include', 'mate_engine.h')) as fh:
        header = fh.read()
    assert re.search(r'int\s+mate_engine_enable_first_rows\s*\(\s*mate_engine\s*\*\s*engine\s*,\s*const\s+mate_first_rows\s*\*\s*config\s*\)', header)
    assert '#define MATE_ABI_VERSION 1' in header                      # additive: the ABI number stays
    # the struct as the header spells it: three pointers in this order
    body = re.search(r'typedef struct mate_first_rows \{(.*?)\} mate_first_rows;', header, re.S).group(1)
    assert re.findall(r'\*\s*(\w+_dev)\s*;', body) == [name for name, _ in _native.MateFirstRows._fields_] == ['rows_dev', 'scalars_dev', 'final_obs_dev']
    assert ctypes.sizeof(_native.MateFirstRows) == 3 * ctypes.sizeof(ctypes.c_void_p)

    from mate_amd.engine import Engine
    from mate_amd.environment import BatchedMultiAgentTracking
    params = inspect.signature(Engine.enable_fragment_rows).parameters
    assert params['first_rows'].default is False and params['final_obs'].default is False
    assert isinstance(Engine.fragment_restarted, property)
    assert inspect.signature(BatchedMultiAgentTracking.__init__).parameters['first_rows'].default is False
