"""clickdeb.tarCreate and ClickDeb.Unpack, GPU-backed (reference clickdeb/deb.go:261-344, 188-203).

Same name, argument meaning and error behaviour as the Go function: tarCreate(tarname, sourceDir, fn) walks
sourceDir, asks fn(path) for every regular file, symlink and directory (False leaves it out; None keeps all),
writes members "./<relative path>" owned by root through gzip into tarname, and raises on the first error.
tarCreate writes ".gz" only: the reference's ".xz" branch shells out to an external tool.  Unpack reads
data.tar.gz, UnpackBz2 data.tar.bz2.  Test/bench harness, like
helpers.py and hashes.py: the product is the C ABI.
"""
from .helpers import default_context


def tarCreate(tarname, sourceDir, fn=None, ctx=None):
    """-> the 64-byte SHA-512 of the archive written (the Go function returns only the error)."""
    _, digest = (ctx or default_context()).tar_create_fn(tarname, sourceDir, fn)
    return digest


def Unpack(dataTarGz, targetDir, hashesYaml=None, ctx=None):
    """ClickDeb.Unpack (clickdeb/deb.go:188-203) of the package's data.tar.gz into targetDir: helpers.UnpackTar with
    clickVerifyContentFn, raising on the first error (SnaphashError: EFORMAT for a corrupt stream, ECONTENT for a ".."
    name or an unsupported member type).  hashesYaml (bytes): also the install-time Verify, from the decoded bytes.
    -> None, or (kind, name) of the first mismatch against hashesYaml."""
    mismatch, _ = (ctx or default_context()).tar_unpack(dataTarGz, targetDir, hashesYaml)
    return mismatch


def UnpackBz2(dataTarBz2, targetDir, hashesYaml=None, ctx=None):
    """ClickDeb.Unpack of a package whose data member is data.tar.bz2 (skipToArMember's ".bz2" branch, clickdeb/deb.go:
    408-441): the same rules, errors and Verify as Unpack, from the bzip2-decoded stream.
    -> None, or (kind, name) of the first mismatch against hashesYaml."""
    mismatch, _ = (ctx or default_context()).tar_unpack_bz2(dataTarBz2, targetDir, hashesYaml)
    return mismatch
