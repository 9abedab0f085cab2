"""Every AV_* environment switch the sources read is documented in INTEGRATION.md's switch table, and the table names no switch
that nothing reads: an experiment's switch is either documented or removed before it is merged."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# error codes (AV_E_*, AV_OK) and the engine flag AV_FE_INPUTS_PERSIST are not switches
NOT_A_SWITCH = re.compile(r'^AV_(E_[A-Z0-9_]+|OK|FE_INPUTS_PERSIST)$')


def _read(path):
    with open(path, encoding='utf-8') as f:
        return f.read()


def switches_read_by_the_library():
    names = set()
    for path in glob.glob(os.path.join(ROOT, 'uav_airvision_amd', 'csrc', '*')):
        names.update(re.findall(r'getenv\("(AV_[A-Z0-9_]+)"', _read(path)))
    return names


def switches_read_by_bench():
    src = _read(os.path.join(ROOT, 'bench.py'))
    names = set(re.findall(r'''os\.environ(?:\.get\(|\[)\s*['"](AV_[A-Z0-9_]+)['"]''', src))
    names.update(re.findall(r'''['"](AV_[A-Z0-9_]+)['"]\s+(?:not\s+)?in\s+os\.environ''', src))
    return names


def switches_in_the_table():
    names = set()
    for line in _read(os.path.join(ROOT, 'INTEGRATION.md')).splitlines():
        if line.startswith('|'):
            names.update(n for n in re.findall(r'AV_[A-Z0-9_]*[A-Z0-9]', line) if not NOT_A_SWITCH.match(n))
    return names


def test_switch_table_matches_the_sources():
    lib, bench = switches_read_by_the_library(), switches_read_by_bench()
    assert lib and bench, 'the patterns found no switch at all'
    read, table = lib | bench, switches_in_the_table()
    assert read == table, 'read but not in the table: %s; in the table but not read: %s' % (sorted(read - table), sorted(table - read))
