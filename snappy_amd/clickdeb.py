"""clickdeb.tarCreate and ClickDeb.Unpack, GPU-backed (reference clickdeb/deb.go:261-344, 188-203).

Same name, argument meaning and error behaviour as the Go function: tarCreate(tarname, sourceDir, fn) walks
sourceDir, asks fn(path) for every regular file, symlink and directory (False leaves it out; None keeps all),
writes members "./<relative path>" owned by root through gzip into tarname, and raises on the first error.
tarCreate dispatches on the suffix as deb.go:269-276 does: ".gz" to the gzip producer, ".xz" (which the reference pipes
through the xz tool) to the library's own .xz producer; anything else is "unknown compression extension".  Unpack reads
data.tar.gz, UnpackBz2 data.tar.bz2, UnpackXz data.tar.xz; ClickDeb opens the .snap itself (clickdeb/deb.go:108-203)
and ClickDeb.create(path).build(dir) writes one (deb.go:346-406).  Test/bench harness, like
helpers.py and hashes.py: the product is the C ABI.
"""
from .helpers import default_context


def tarCreate(tarname, sourceDir, fn=None, ctx=None, self_check=False, filter=None):
    """-> the 64-byte SHA-512 of the archive written (the Go function returns only the error).  self_check (".xz" names
    only): the producer walks every LZMA2 chunk against the bytes it was made from before it leaves the GPU.  filter
    (".xz" names only): a BCJ filter in front of LZMA2 -- "x86", "arm" or "armthumb", what the reference's xz writes when
    XZ_OPT names one; UnpackXz(..., bcj=True) reads the file back."""
    c = ctx or default_context()
    if str(tarname).endswith(".xz"):
        if fn is not None:
            raise ValueError("tarCreate: the .xz producer takes no exclude function (snaphash_tar_create_xz)")
        return c.tar_create_xz(tarname, sourceDir, self_check=self_check, filter=filter)[1]
    if self_check:
        raise ValueError("tarCreate: self_check is the .xz producer's (ClickDeb.build(check=True) is the .gz producer's)")
    if filter:
        raise ValueError("tarCreate: filter is the .xz producer's")
    _, digest = c.tar_create_fn(tarname, sourceDir, fn)  # (any suffix but ".gz": SnaphashError, "unknown compression extension")
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


def UnpackXz(dataTarXz, targetDir, hashesYaml=None, ctx=None, bcj=False, chains=False):
    """ClickDeb.Unpack of a package whose data member is data.tar.xz (skipToArMember's ".xz" branch, clickdeb/deb.go:
    408-441): the same rules, errors and Verify as Unpack, from the xz-decoded stream.  A filter chain or Check the
    decoder does not take raises SnaphashError with code EINVAL.  bcj: Blocks with an x86, ARM or ARM-Thumb filter in front
    of LZMA2 are taken too (what tarCreate(..., filter=) writes); chains: every chain liblzma reads.
    -> None, or (kind, name) of the first mismatch against hashesYaml."""
    mismatch, _ = (ctx or default_context()).tar_unpack_xz(dataTarXz, targetDir, hashesYaml, bcj=bcj, chains=chains)
    return mismatch


class ClickDeb:
    """The reference's ClickDeb on a .snap file (clickdeb/deb.go:108-203): the ar container read once, control.tar.* and
    data.tar.* decoded at most once each however many calls follow.  ClickDeb.open(path) as the Go Open; a context manager."""

    def __init__(self, snap):
        self._snap = snap

    @classmethod
    def open(cls, path, ctx=None, xz=False, chains=False):
        """xz: control.tar.xz / data.tar.xz members are read too, through the library's .xz engine (the reference pipes them
        through the xz tool); without it they raise SnaphashError EINVAL "Can not handle ...", as they always did.  chains
        (with xz): their Blocks may carry any filter chain liblzma reads, Delta, PowerPC, IA64 and SPARC among them."""
        return cls((ctx or default_context()).snap_open(path, xz=xz, chains=chains))

    @classmethod
    def create(cls, path, ctx=None):
        """clickdeb.Create(path): the package to be written by build().  (The file appears when build() runs.)"""
        return ClickDebWriter(path, ctx or default_context())

    def close(self):
        self._snap.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def members(self):
        """-> [(name, offset, size)] of the ar members."""
        return self._snap.members()

    def control_member(self, name):
        """ClickDeb.ControlMember: the content of `name` in control.tar.* (None when absent)."""
        return self._snap.control_member(name)

    def meta_member(self, name):
        """ClickDeb.MetaMember: the content of meta/<name> in data.tar.* (None when absent)."""
        return self._snap.meta_member(name)

    def unpack(self, targetDir, verify=True):
        """ClickDeb.Unpack into targetDir, with the install-time Verify against the package's own hashes.yaml.
        -> None, or (kind, name) of the first mismatch."""
        return self._snap.unpack(targetDir, verify)[0]

    def audit(self):
        """Every check the package carries (CRCs, archive-sha512, every record of hashes.yaml), nothing written.
        -> None, or (kind, name) of the first mismatch."""
        return self._snap.audit()[0]

    def stats(self):
        return self._snap.stats()


class ClickDebWriter:
    """What ClickDeb.create returns: Build (clickdeb/deb.go:346-406) with snappy.Build's writeHashes callback fused in."""

    def __init__(self, path, ctx):
        self.path = path
        self._ctx = ctx
        self.archive_digest = self.snap_digest = self.build_stats = None

    def build(self, sourceDir, hashes=True, check=False, mtime=-1, codec="gz", **codec_options):
        """ClickDeb.Build(sourceDir, callback): the data member from one read of the tree, DEBIAN/hashes.yaml from the same
        pass (hashes=False: the nil callback), control.tar.gz, the ar container.  codec: "gz" (data.tar.gz, what the
        reference hard-codes), "xz" or "bz2" -- the member is then what tarCreate's producer of that name writes;
        codec_options: block_size, xz_check, filter, level for "xz", level for "bz2" (Context.snap_build).  check=True:
        what was compressed is decoded again in HBM and compared with what it was made from before it is written -- the
        DEFLATE chunks of control.tar.gz and of a data.tar.gz, the LZMA2 chunks of a data.tar.xz, the blocks of a
        data.tar.bz2.  Raises SnaphashError and leaves no file on failure.  -> self; archive_digest, snap_digest (the
        store's download_sha512) and build_stats are set.  ClickDeb.open(path, xz=True) reads a data.tar.xz back."""
        self.archive_digest, self.snap_digest, self.build_stats = self._ctx.snap_build(sourceDir, self.path, hashes, check, mtime, codec,
                                                                                       **codec_options)
        return self

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
