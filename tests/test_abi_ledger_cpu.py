"""The table of extension headers (abi_ledger.HEADERS) against mmft.lib and the built library, one case per accessor: what
the per-header ledgers assert about their own header, asserted of every header against every other one."""
import pytest

from abi_ledger import HEADERS, declared, others
from mmft import lib


def test_the_table_lists_exactly_the_header_instances_of_lib():
    found = {k: v for k, v in vars(lib).items() if isinstance(v, lib.Header)}
    assert set(found) == set(HEADERS)
    assert len({id(v) for v in found.values()}) == len(HEADERS) == len(set(HEADERS.values())) == 9
    for acc, header in HEADERS.items():
        assert found[acc].path.replace('\\', '/').endswith('include/' + header), acc
        assert getattr(lib, acc + '_decls') == found[acc].decls
        assert found[acc] not in (lib.call, lib.query)


@pytest.mark.parametrize('acc', list(HEADERS))
def test_accessor_binds_its_own_header_and_refuses_every_other(acc):
    header, accessor = HEADERS[acc], getattr(lib, acc)
    mine, decls = declared(header), accessor.decls()
    assert mine and {n: len(args) for n, (_, args) in decls.items()} == mine
    with pytest.raises(RuntimeError, match='not declared'):
        accessor('mmft_version')
    for other in others(header):
        theirs = declared(other)
        assert theirs and not set(mine) & set(theirs), other
        with pytest.raises(RuntimeError, match=f'{sorted(theirs)[0]} is not declared in .*{header}'):
            accessor(sorted(theirs)[0])
    L = lib.load()
    assert not [n for n in mine if not hasattr(L, n)]
