package rnabloom.graph;

import java.io.*;
import java.nio.ByteBuffer;
import java.util.*;
import rnabloom.bloom.BloomFilter;
import rnabloom.bloom.CountingBloomFilter;
import rnabloom.bloom.hash.*;
import static rnabloom.util.SeqUtils.*;

/**
 * Drop-in for the reference's rnabloom.graph.BloomFilterDeBruijnGraph (src/rnabloom/graph/BloomFilterDeBruijnGraph.java):
 * the same constructors, the same public methods, the same files on disk — with the four filters resident in HBM behind ONE
 * rb_graph handle (librb_hip.so through NativeGraph) instead of four Unsafe*Buffers.
 *
 * What changes for callers: nothing in the signatures.  Per-element methods (add(long[]), contains(long[]), getCount(long[]),
 * ...) call the batched natives with n = 1, so code that is not ported yet keeps working; the hot loops should move to the
 * batched forms at the end of this class (applyAll / containsAll / getCountAll) and stage 1 to
 * NativeGraph.addReads / addFastq (see NativeFastqToGraphWorker in this directory).  Only hashVals[0] crosses the boundary: the
 * library re-derives hashVals[1..] with NTM64 from the graph's k (src/rnabloom/bloom/hash/NTHash.java:518-527) — which is
 * what every hashVals array in the reference was made with.
 *
 * Kmer and CanonicalKmer have drop-ins beside this file (one NativeGraph.neighbors call per k-mer neighbourhood); HashFunction and the
 * iterators stay the reference's own classes.  (HashFunction needs one accessor the reference does not have:
 * `public int getK() { return k; }`.)
 */
public class BloomFilterDeBruijnGraph {
    private long handle;                                   // rb_graph*: dbgbf, cbf, rpkbf, fpkbf live on the device behind it
    private BloomFilter dbgbf, rpkbf, fpkbf;               // thin views of the handle's filters (getDbgbf() etc.); null = absent
    private CountingBloomFilter cbf;
    private final HashFunction hashFunction;
    private int k, kMinus1;
    private boolean stranded;
    private int dbgbfNumHash, cbfNumHash, pkbfNumHash, dbgbfCbfMaxNumHash;
    private int readPairedKmersDistance = -1, fragmentPairedKmersDistance = -1;

    private static final String EXT_DESC = ".desc", EXT_DBGBF = ".dbgbf", EXT_CBF = ".cbf", EXT_FPKBF = ".fpkbf", EXT_RPKBF = ".rpkbf";

    public BloomFilterDeBruijnGraph(long dbgbfNumBits, long cbfNumBytes, long pkbfNumBits, int dbgbfNumHash, int cbfNumHash, int pkbfNumHash,
                                    int k, boolean stranded, boolean useReadPairedKmers) {
        this.k = k; this.kMinus1 = k - 1; this.stranded = stranded;
        this.dbgbfNumHash = dbgbfNumHash; this.cbfNumHash = cbfNumHash; this.pkbfNumHash = pkbfNumHash;
        this.dbgbfCbfMaxNumHash = dbgbfNumHash > cbfNumHash ? dbgbfNumHash : cbfNumHash;
        this.hashFunction = stranded ? new HashFunction(k) : new CanonicalHashFunction(k);
        this.handle = NativeGraph.create(dbgbfNumBits, cbfNumBytes, pkbfNumBits, dbgbfNumHash, cbfNumHash, pkbfNumHash, k, stranded,
                                         useReadPairedKmers, NativeGraph.defaultDevice(), 0L);
        this.dbgbf = new BloomFilter(handle, NativeGraph.DBGBF, dbgbfNumBits, dbgbfNumHash, hashFunction);
        this.cbf = new CountingBloomFilter(handle, cbfNumBytes, cbfNumHash, hashFunction);
        this.rpkbf = useReadPairedKmers ? new BloomFilter(handle, NativeGraph.RPKBF, pkbfNumBits, pkbfNumHash, hashFunction) : null;
    }

    private static HashMap<String, String> readLabels(File f) throws IOException {
        HashMap<String, String> m = new HashMap<>();
        try (BufferedReader br = new BufferedReader(new FileReader(f))) {
            for (String line = br.readLine(); line != null; line = br.readLine()) {
                String[] kv = line.split(":");
                if (kv.length >= 2) m.put(kv[0], kv[1]);
            }
        }
        return m;
    }

    public void updateFragmentKmerDistance(File graphFile) throws FileNotFoundException, IOException {
        String v = readLabels(graphFile).get("fragmentPairedKmersDistance");
        if (v != null) {
            fragmentPairedKmersDistance = Integer.parseInt(v);
            NativeGraph.setFragPairedKmerDistance(handle, fragmentPairedKmersDistance);
        }
    }

    public BloomFilterDeBruijnGraph(File graphFile, boolean loadDbgBits) throws FileNotFoundException, IOException {
        HashMap<String, String> d = readLabels(graphFile);
        if (d.containsKey("dbgbfCbfMaxNumHash")) dbgbfCbfMaxNumHash = Integer.parseInt(d.get("dbgbfCbfMaxNumHash"));
        if (d.containsKey("k")) { k = Integer.parseInt(d.get("k")); kMinus1 = k - 1; }
        if (d.containsKey("stranded")) stranded = Boolean.parseBoolean(d.get("stranded"));
        if (d.containsKey("fragmentPairedKmersDistance")) fragmentPairedKmersDistance = Integer.parseInt(d.get("fragmentPairedKmersDistance"));
        if (d.containsKey("readPairedKmersDistance")) readPairedKmersDistance = Integer.parseInt(d.get("readPairedKmersDistance"));
        this.hashFunction = stranded ? new HashFunction(k) : new CanonicalHashFunction(k);

        String base = graphFile.getPath();
        long[] dDesc = BloomFilter.readDesc(new File(base + EXT_DBGBF + EXT_DESC));
        long[] cDesc = BloomFilter.readDesc(new File(base + EXT_CBF + EXT_DESC));
        File rBits = new File(base + EXT_RPKBF), rDesc = new File(base + EXT_RPKBF + EXT_DESC);
        File fBits = new File(base + EXT_FPKBF), fDesc = new File(base + EXT_FPKBF + EXT_DESC);
        boolean hasR = rBits.isFile() && rDesc.isFile(), hasF = fBits.isFile() && fDesc.isFile();
        long[] rD = hasR ? BloomFilter.readDesc(rDesc) : new long[]{0, 1};
        dbgbfNumHash = (int) dDesc[1];
        cbfNumHash = (int) cDesc[1];
        handle = NativeGraph.create(dDesc[0], cDesc[0], rD[0], dbgbfNumHash, cbfNumHash, (int) rD[1], k, stranded, hasR, NativeGraph.defaultDevice(), 0L);
        dbgbf = new BloomFilter(handle, NativeGraph.DBGBF, dDesc[0], dbgbfNumHash, hashFunction);
        cbf = new CountingBloomFilter(handle, cDesc[0], cbfNumHash, hashFunction);
        if (loadDbgBits) importFile(NativeGraph.DBGBF, new File(base + EXT_DBGBF));
        importFile(NativeGraph.CBF, new File(base + EXT_CBF));
        if (hasF) {
            long[] fD = BloomFilter.readDesc(fDesc);
            pkbfNumHash = (int) fD[1];
            NativeGraph.initFragmentPairs(handle, fD[0], pkbfNumHash);
            fpkbf = new BloomFilter(handle, NativeGraph.FPKBF, fD[0], pkbfNumHash, hashFunction);
            importFile(NativeGraph.FPKBF, fBits);
        }
        if (hasR) {
            pkbfNumHash = (int) rD[1];
            rpkbf = new BloomFilter(handle, NativeGraph.RPKBF, rD[0], pkbfNumHash, hashFunction);
            importFile(NativeGraph.RPKBF, rBits);
        }
        if (readPairedKmersDistance >= 0) NativeGraph.setReadPairedKmerDistance(handle, readPairedKmersDistance);
        if (fragmentPairedKmersDistance >= 0) NativeGraph.setFragPairedKmerDistance(handle, fragmentPairedKmersDistance);
    }

    private void importFile(int which, File bytes) throws IOException {
        long n = NativeGraph.filterSize(handle, which)[1];
        NativeGraph.importFilterFromFile(handle, which, bytes.getPath(), n);
    }

    /** the rb_graph handle, for the batched natives (NativeGraph.addReads, addFastq, batchCounts, walk, ...) */
    public long getHandle() { return handle; }

    public HashFunction getHashFunction() { return this.hashFunction; }

    public int getDbgbfNumHash() { return dbgbfNumHash; }

    public int getCbfNumHash() { return cbfNumHash; }

    public int getPkbfNumHash() { return pkbfNumHash; }

    public int getMaxNumHash() { return dbgbfCbfMaxNumHash; }

    public void destroy() {
        if (handle != 0) { NativeGraph.destroy(handle); handle = 0; }
        dbgbf = null; cbf = null; rpkbf = null; fpkbf = null;
    }

    public void clearAllBf() { NativeGraph.clear(handle, 15); }

    public void clearDbgbf() { NativeGraph.clear(handle, 1 << NativeGraph.DBGBF); }

    public void clearCbf() { NativeGraph.clear(handle, 1 << NativeGraph.CBF); }

    public void clearFpkbf() { if (fpkbf != null) NativeGraph.clear(handle, 1 << NativeGraph.FPKBF); }

    public void clearRpkbf() { if (rpkbf != null) NativeGraph.clear(handle, 1 << NativeGraph.RPKBF); }

    public void destroyDbgbf() { if (dbgbf != null) { NativeGraph.destroyFilter(handle, NativeGraph.DBGBF); dbgbf = null; } }

    public void destroyCbf() { if (cbf != null) { NativeGraph.destroyFilter(handle, NativeGraph.CBF); cbf = null; } }

    public void destroyFpkbf() { if (fpkbf != null) { NativeGraph.destroyFilter(handle, NativeGraph.FPKBF); fpkbf = null; } }

    public void destroyRpkbf() { if (rpkbf != null) { NativeGraph.destroyFilter(handle, NativeGraph.RPKBF); rpkbf = null; } }

    public BloomFilter getDbgbf() { return dbgbf; }

    public CountingBloomFilter getCbf() { return cbf; }

    public BloomFilter getFpkbf() { return fpkbf; }

    public BloomFilter getRpkbf() { return rpkbf; }

    public boolean isStranded() { return stranded; }

    public void saveDesc(File graphFile) throws IOException {
        try (FileWriter w = new FileWriter(graphFile)) {
            w.write("dbgbfCbfMaxNumHash:" + dbgbfCbfMaxNumHash + "\n" + "stranded:" + stranded + "\n" + "k:" + k + "\n"
                    + "readPairedKmersDistance:" + readPairedKmersDistance + "\n"
                    + "fragmentPairedKmersDistance:" + fragmentPairedKmersDistance + "\n");
        }
    }

    public void save(File graphFile) throws IOException {
        saveDesc(graphFile);
        String base = graphFile.getPath();
        dbgbf.save(new File(base + EXT_DBGBF + EXT_DESC), new File(base + EXT_DBGBF));
        cbf.save(new File(base + EXT_CBF + EXT_DESC), new File(base + EXT_CBF));
        if (rpkbf != null) rpkbf.save(new File(base + EXT_RPKBF + EXT_DESC), new File(base + EXT_RPKBF));
    }

    public void savePkbf(File graphFile) throws IOException {
        saveDesc(graphFile);                       // the k-mer pair distance may have changed
        String base = graphFile.getPath();
        fpkbf.save(new File(base + EXT_FPKBF + EXT_DESC), new File(base + EXT_FPKBF));
    }

    public void restorePkbf(File graphFile) throws IOException {
        String base = graphFile.getPath();
        long[] fD = BloomFilter.readDesc(new File(base + EXT_FPKBF + EXT_DESC));
        if (fpkbf != null) NativeGraph.destroyFilter(handle, NativeGraph.FPKBF);
        pkbfNumHash = (int) fD[1];
        NativeGraph.initFragmentPairs(handle, fD[0], pkbfNumHash);
        fpkbf = new BloomFilter(handle, NativeGraph.FPKBF, fD[0], pkbfNumHash, hashFunction);
        importFile(NativeGraph.FPKBF, new File(base + EXT_FPKBF));
    }

    public void initializePairKmersBloomFilter(long pkbfNumBits, int pkbfNumHash) {
        if (fpkbf == null) {
            this.pkbfNumHash = pkbfNumHash;
            NativeGraph.initFragmentPairs(handle, pkbfNumBits, pkbfNumHash);
            fpkbf = new BloomFilter(handle, NativeGraph.FPKBF, pkbfNumBits, pkbfNumHash, hashFunction);
        } else {
            fpkbf.empty();
        }
    }

    public void setFragPairedKmerDistance(int d) { fragmentPairedKmersDistance = d; NativeGraph.setFragPairedKmerDistance(handle, d); }

    public int getFragPairedKmerDistance() { return fragmentPairedKmersDistance; }

    public void setReadPairedKmerDistance(int d) { readPairedKmersDistance = d; NativeGraph.setReadPairedKmerDistance(handle, d); }

    public int getReadPairedKmerDistance() { return readPairedKmersDistance; }

    public int getK() { return k; }

    /** the handle keeps the k it was created with (it salts NTM64): as in the reference, iterators made before a setK keep theirs */
    public void setK(int k) {
        this.k = k;
        this.kMinus1 = k - 1;
        this.hashFunction.setK(k);
    }

    public int getKMinus1() { return kMinus1; }

    public boolean isLowComplexity(Kmer kmer) { return isLowComplexity2(kmer.bytes); }

    public boolean isRepeatKmer(Kmer kmer) { return isRepeat(kmer.bytes); }

    // ---- per-element mutators: one native call with n = 1 (src/.../BloomFilterDeBruijnGraph.java:399-461) ----
    private static long[] one(long v) { return new long[]{v}; }

    private long[] hashesOf(String kmer) {
        final long[] h = new long[dbgbfCbfMaxNumHash];
        hashFunction.getHashValues(kmer, h.length, h);
        return h;
    }

    public void add(String kmer) { add(hashesOf(kmer)); }

    public void add(final long[] hashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD, one(hashVals[0]), 1); }

    public void addIfAbsent(final long[] hashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD_IF_ABSENT, one(hashVals[0]), 1); }

    public void addCountIfPresent(final long[] hashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD_COUNT_IF_PRESENT, one(hashVals[0]), 1); }

    public void addDbgOnly(final long hashVal) { NativeGraph.apply(handle, NativeGraph.OP_ADD_DBG_ONLY, one(hashVal), 1); }

    public void addDbgOnly(final long[] hashVals) { addDbgOnly(hashVals[0]); }

    public void addCountOnly(final long[] hashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD_COUNT_ONLY, one(hashVals[0]), 1); }

    public void addReadSingleKmerPair(long[] pairingHashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD_READ_PAIR, one(pairingHashVals[0]), 1); }

    public void addFragmentSingleKmerPair(long[] pairingHashVals) { NativeGraph.apply(handle, NativeGraph.OP_ADD_FRAG_PAIR, one(pairingHashVals[0]), 1); }

    /** hashVals[0] of the pair (kmers[i], kmers[i + d]) for i < kmers.size() - d: what the four methods below hand to a pair filter */
    private long[] pairHashes(ArrayList<Kmer> kmers, int d) {
        final int n = kmers.size() - d;
        if (n <= 0) return new long[0];
        long[] h = new long[n];
        for (int i = 0; i < n; ++i) h[i] = kmers.get(i).getKmerPairHashValue(kmers.get(i + d));
        return h;
    }

    public void addFragmentPairKmers(ArrayList<Kmer> kmers) {
        long[] h = pairHashes(kmers, fragmentPairedKmersDistance);
        if (h.length > 0) NativeGraph.apply(handle, NativeGraph.OP_ADD_FRAG_PAIR, h, h.length);
    }

    public void addReadPairedKmers(ArrayList<Kmer> kmers) {
        long[] h = pairHashes(kmers, readPairedKmersDistance);
        if (h.length > 0) NativeGraph.apply(handle, NativeGraph.OP_ADD_READ_PAIR, h, h.length);
    }

    public boolean containsAllPairedKmers(ArrayList<Kmer> kmers) {
        long[] h = pairHashes(kmers, fragmentPairedKmersDistance);
        if (h.length == 0) return false;
        byte[] o = new byte[h.length];
        NativeGraph.filterLookup(handle, NativeGraph.FPKBF, h, h.length, o);
        for (byte b : o) if (b == 0) return false;
        return true;
    }

    /** one lookupThenAdd over the sequence's pairs IN ORDER (a later pair sees the bits of an earlier one), ANDed — :513-524 */
    public boolean lookupAndAddAllPairedKmers(ArrayList<Kmer> kmers) {
        long[] h = pairHashes(kmers, fragmentPairedKmersDistance);
        if (h.length == 0) return true;
        byte[] o = new byte[h.length];
        NativeGraph.filterLookupThenAdd(handle, NativeGraph.FPKBF, h, h.length, o);
        boolean all = true;
        for (byte b : o) all &= b != 0;
        return all;
    }

    public boolean lookupFragmentKmerPair(Kmer left, Kmer right) { return fpkbf.lookup(left.getKmerPairHashValue(right)); }

    public boolean lookupReadKmerPair(Kmer left, Kmer right) { return rpkbf.lookup(left.getKmerPairHashValue(right)); }

    // ---- queries ----
    public boolean contains(String kmer) { return contains(hashesOf(kmer)); }

    public boolean contains(final long[] hashVals) {
        byte[] o = new byte[1];
        NativeGraph.contains(handle, one(hashVals[0]), 1, o);
        return o[0] != 0;
    }

    public void increment(String kmer) { cbf.increment(kmer); }

    public float getCount(String kmer) { return getCount(hashesOf(kmer)); }

    /** dbgbf.lookup ? cbf.getCount + 1 : 0 (:552-570), evaluated on the device */
    public float getCount(final long hashVal) {
        float[] o = new float[1];
        NativeGraph.getCount(handle, one(hashVal), 1, o);
        return o[0];
    }

    public float getCount(final long[] hashVals) { return getCount(hashVals[0]); }

    public float getDbgbfFPR() { return NativeGraph.fpr(handle, NativeGraph.DBGBF); }

    public float getCbfFPR() { return NativeGraph.fpr(handle, NativeGraph.CBF); }

    public float getRpkbfFPR() { return NativeGraph.fpr(handle, NativeGraph.RPKBF); }

    public float getPkbfFPR() { return NativeGraph.fpr(handle, NativeGraph.FPKBF); }

    public float getFPR() { return getDbgbfFPR() * getCbfFPR(); }

    public Kmer getKmer(String kmer) { return hashFunction.getKmer(kmer, dbgbfCbfMaxNumHash, this); }

    public String getPrefix(String kmer) { return kmer.substring(0, kMinus1); }

    public String getSuffix(String kmer) { return kmer.substring(1, k); }

    public CharSequence getPrefixCharSeq(String kmer) { return kmer.subSequence(0, kMinus1); }

    public CharSequence getSuffixCharSeq(String kmer) { return kmer.subSequence(1, k); }

    /**
     * The k-mers that differ from `kmer` in one END base and are in the graph (:1056-1068, :1113-1124): the alternatives are hashed on
     * the host and looked up with ONE batched native call instead of one `contains` per alternative.
     */
    private ArrayDeque<String> endVariants(String kmer, boolean firstBase) {
        final char[] alts = getAltNucleotides(kmer.charAt(firstBase ? 0 : kMinus1));
        final String[] cand = new String[alts.length];
        final long[] base = new long[alts.length];
        final StringBuilder sb = new StringBuilder(kmer);
        for (int i = 0; i < alts.length; ++i) {
            sb.setCharAt(firstBase ? 0 : kMinus1, alts[i]);
            cand[i] = sb.toString();
            base[i] = hashesOf(cand[i])[0];
        }
        final byte[] present = new byte[alts.length];
        if (alts.length > 0) NativeGraph.contains(handle, base, alts.length, present);
        final ArrayDeque<String> found = new ArrayDeque<>(4);
        for (int i = 0; i < alts.length; ++i) if (present[i] != 0) found.add(cand[i]);
        return found;
    }

    public ArrayDeque<String> getLeftVariants(String kmer) { return endVariants(kmer, true); }

    public ArrayDeque<String> getRightVariants(String kmer) { return endVariants(kmer, false); }

    public float[] getCounts(String[] kmers) {
        long[] h = new long[kmers.length];
        for (int i = 0; i < kmers.length; ++i) h[i] = hashesOf(kmers[i])[0];
        float[] counts = new float[kmers.length];
        if (kmers.length > 0) NativeGraph.getCount(handle, h, h.length, counts);
        return counts;
    }

    /** every k-mer of seq is in dbgbf (:1181-1194): the iterator's base hashes are collected and looked up in one batched call */
    public boolean isValidSeq(String seq) {
        final int windows = seq.length() - k + 1;
        if (windows <= 0) return true;
        final long[] base = new long[windows];
        final NTHashIterator it = getHashIterator();
        it.start(seq);
        int n = 0;
        for (; it.hasNext() && n < windows; ++n) {
            it.next();
            base[n] = it.hVals[0];
        }
        if (n == 0) return true;
        final byte[] present = new byte[n];
        NativeGraph.contains(handle, base, n, present);
        for (int i = 0; i < n; ++i) if (present[i] == 0) return false;
        return true;
    }

    public NTHashIterator getHashIterator() { return hashFunction.getHashIterator(this.dbgbfCbfMaxNumHash); }

    public NTHashIterator getHashIterator(int numHash) { return hashFunction.getHashIterator(numHash); }

    public NTHashIterator getHashIterator(int numHash, int k) { return hashFunction.getHashIterator(numHash, k); }

    public NTHashIterator getReverseComplementHashIterator(int numHash) { return hashFunction.getReverseComplementHashIterator(numHash); }

    public NTHashIterator getReverseComplementHashIterator(int numHash, int k) { return hashFunction.getReverseComplementHashIterator(numHash, k); }

    public PairedNTHashIterator getPairedHashIterator(int d) { return hashFunction.getPairedHashIterator(this.pkbfNumHash, d); }

    public PairedNTHashIterator getReverseComplementPairedHashIterator(int d) { return hashFunction.getReverseComplementPairedHashIterator(this.pkbfNumHash, d); }

    /**
     * getKmers (:1224-1234 -> {Canonical,}HashFunction.getKmers, src/rnabloom/bloom/hash/CanonicalHashFunction.java:46-170): the
     * reference hashes window by window and asks graph.getCount per k-mer — here ONE NativeGraph.getKmers call returns forward hash,
     * reverse hash and count of every window of seq[start, end) (count 0 for a window with a character outside ACGTU, :73-78), and the
     * Kmer objects are built from the arrays.  Kmer / CanonicalKmer are the reference's own classes.
     */
    private static final class WindowProfile {
        final byte[] bytes; final long[] f, r; final float[] count; final int n;
        WindowProfile(byte[] bytes, long[] f, long[] r, float[] count, int n) { this.bytes = bytes; this.f = f; this.r = r; this.count = count; this.n = n; }
    }

    private WindowProfile profile(String seq, int start, int end) {
        final int len = end - start, n = len - k + 1;
        final byte[] ascii = new byte[Math.max(len, 0)];
        for (int i = 0; i < len; ++i) ascii[i] = (byte) seq.charAt(start + i);
        if (n <= 0) return new WindowProfile(ascii, new long[0], new long[0], new float[0], 0);
        final ByteBuffer text = ByteBuffer.allocateDirect(len);
        text.put(ascii);
        final long[] f = new long[n], r = new long[n], koff = new long[2];
        final float[] count = new float[n];
        NativeGraph.getKmers(handle, text, new long[]{0L, (long) len}, 1, koff, f, r, count);
        return new WindowProfile(ascii, f, r, count, n);
    }

    private Kmer kmerAt(WindowProfile w, int i) {
        final byte[] b = Arrays.copyOfRange(w.bytes, i, i + k);
        return stranded ? new Kmer(b, w.count[i], w.f[i]) : new CanonicalKmer(b, w.count[i], w.f[i], w.r[i]);
    }

    /**
     * GraphUtils.correctMismatches (src/rnabloom/util/GraphUtils.java:3914-3996) for a batch of sequences in ONE native call: the two scans
     * run on the device, a wavefront per sequence.  covThresholds[i] is sequence i's covThreshold.  Returns the corrected sequences;
     * nFixed[i] (optional, seqs.length entries) receives the number of replacements — the reference's `corrected` is nFixed[i] > 0.
     */
    public String[] correctMismatches(String[] seqs, float[] covThresholds, float minKmerCov, int[] nFixed) {
        final int n = seqs.length;
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        final int total = (int) off[n];
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max(total, 1)), out = ByteBuffer.allocateDirect(Math.max(total, 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        final int[] fixed = nFixed != null ? nFixed : new int[n];
        NativeGraph.correctMismatches(handle, text, off, n, covThresholds, minKmerCov, out, fixed, null, null);
        final String[] res = new String[n];
        final byte[] b = new byte[total];
        out.get(b, 0, total);
        for (int i = 0; i < n; ++i)
            res[i] = fixed[i] > 0 ? new String(b, (int) off[i], (int) (off[i + 1] - off[i]), java.nio.charset.StandardCharsets.ISO_8859_1) : seqs[i];
        return res;
    }

    /**
     * GraphUtils.correctErrorHelper (src/rnabloom/util/GraphUtils.java:3711-3912) for a batch of sequences in ONE native call: the gap scan, the
     * three repair rules and correctMismatches run on the device.  covThresholds[i] is sequence i's covThreshold.  Returns, per sequence, the
     * string the reference's returned k-mers spell, or null where the reference returns null (nothing was corrected).
     */
    public String[] correctErrors(String[] seqs, float[] covThresholds, int lookahead, int maxIndelSize, float percentIdentity, float minKmerCov) {
        final int n = seqs.length;
        final long[] off = new long[n + 1], outOff = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("correctErrors: more than 2 GB of text in one batch");
        final int total = (int) off[n];
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max(total, 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        // (the native throws IllegalArgumentException when the capacity layout outgrows an int)
        final int cap = NativeGraph.correctErrors(handle, text, off, n, covThresholds, lookahead, maxIndelSize, percentIdentity, minKmerCov, outOff, null,
                                                  null, null, null, null);
        final ByteBuffer out = ByteBuffer.allocateDirect(Math.max(cap, 1));
        final int[] len = new int[n], flags = new int[n];
        NativeGraph.correctErrors(handle, text, off, n, covThresholds, lookahead, maxIndelSize, percentIdentity, minKmerCov, outOff, out, len, flags, null,
                                  null);
        final byte[] b = new byte[cap];
        out.get(b, 0, cap);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = (flags[i] & 1) != 0 ? new String(b, (int) outOff[i], len[i], java.nio.charset.StandardCharsets.ISO_8859_1) : null;
        return res;
    }

    /**
     * GraphUtils.overlap (src/rnabloom/util/GraphUtils.java:4898-5063) for a batch of read pairs in ONE native call: the suffix / prefix match,
     * the dovetail attempt and the spanning k-mers' look-ups run on the device, a wavefront per pair, and nothing is written to the graph.
     * Returns, per pair, the string the reference's returned k-mers spell, or null where the reference returns null (the cue for join).
     * recs (optional, 8 * lefts.length ints) receives the records of NativeGraph.overlapPairs: a pair whose outcome recs[8 i] is 5 is one the
     * reference would rescue — its string is the joined text BEFORE lines :5018-5056, which the caller runs on that pair's Kmer lists.
     */
    public String[] overlapPairs(String[] lefts, String[] rights, int minOverlap, float minKmerCov, int[] recs) {
        final int n = lefts.length;
        if (rights.length != n) throw new IllegalArgumentException("overlapPairs: " + n + " left reads and " + rights.length + " right reads");
        final long[] lo = new long[n + 1], ro = new long[n + 1], outOff = new long[n + 1];
        for (int i = 0; i < n; ++i) { lo[i + 1] = lo[i] + lefts[i].length(); ro[i + 1] = ro[i] + rights[i].length(); }
        if (lo[n] + ro[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("overlapPairs: more than 2 GB of text in one batch");
        final ByteBuffer lt = ByteBuffer.allocateDirect(Math.max((int) lo[n], 1)), rt = ByteBuffer.allocateDirect(Math.max((int) ro[n], 1));
        for (String s : lefts) for (int i = 0; i < s.length(); ++i) lt.put((byte) s.charAt(i));
        for (String s : rights) for (int i = 0; i < s.length(); ++i) rt.put((byte) s.charAt(i));
        final int cap = (int) (lo[n] + ro[n]);
        final ByteBuffer out = ByteBuffer.allocateDirect(Math.max(cap, 1));
        final int[] rec = recs != null ? recs : new int[8 * n];
        NativeGraph.overlapPairs(handle, lt, lo, rt, ro, n, minOverlap, minKmerCov, outOff, out, rec);
        final byte[] b = new byte[cap];
        out.get(b, 0, cap);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = rec[8 * i] != 0 ? new String(b, (int) outOff[i], rec[8 * i + 4], java.nio.charset.StandardCharsets.ISO_8859_1) : null;
        return res;
    }

    /**
     * GraphUtils.join (src/rnabloom/util/GraphUtils.java:892-1147) for a batch of read pairs in ONE native call — the pairs overlapPairs returned
     * null for: both walks, their membership tests and the branch steps at forks run on the device, a wavefront per pair, and nothing is
     * written to the graph.  lookahead, maxIndelLen and minPercentIdentity of the reference's signature are never read by its body and are not
     * parameters here.  Returns, per pair, the string the reference's returned k-mers spell, or null where the reference returns null and
     * where the pair cannot be judged (a read shorter than k, a letter outside ACGTU: records[12 i] == 2).  records (optional, 12 *
     * lefts.length ints) receives the records of NativeGraph.joinPairs.
     */
    public String[] joinPairs(String[] lefts, String[] rights, int bound, float maxCovGradient, int maxTipLen, float minKmerCov, int[] records) {
        final int n = lefts.length;
        if (rights.length != n) throw new IllegalArgumentException("joinPairs: " + n + " left reads and " + rights.length + " right reads");
        if (records != null && records.length < 12L * n) throw new IllegalArgumentException("joinPairs: records holds " + records.length + " ints, " + 12L * n + " are needed");
        if (12L * n > Integer.MAX_VALUE) throw new IllegalArgumentException("joinPairs: " + n + " pairs' records do not fit one array: smaller batches");
        final long[] lo = new long[n + 1], ro = new long[n + 1], outOff = new long[n + 1];
        for (int i = 0; i < n; ++i) { lo[i + 1] = lo[i] + lefts[i].length(); ro[i + 1] = ro[i] + rights[i].length(); }
        if (lo[n] + ro[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("joinPairs: more than 2 GB of text in one batch");
        final ByteBuffer lt = ByteBuffer.allocateDirect(Math.max((int) lo[n], 1)), rt = ByteBuffer.allocateDirect(Math.max((int) ro[n], 1));
        for (String s : lefts) for (int i = 0; i < s.length(); ++i) lt.put((byte) s.charAt(i));
        for (String s : rights) for (int i = 0; i < s.length(); ++i) rt.put((byte) s.charAt(i));
        final int[] rec = records != null ? records : new int[12 * n];
        final int cap = NativeGraph.joinPairs(handle, lt, lo, rt, ro, n, bound, maxCovGradient, maxTipLen, minKmerCov, outOff, null, null);
        final ByteBuffer out = ByteBuffer.allocateDirect(Math.max(cap, 1));
        NativeGraph.joinPairs(handle, lt, lo, rt, ro, n, bound, maxCovGradient, maxTipLen, minKmerCov, outOff, out, rec);
        final byte[] b = new byte[cap];
        out.get(b, 0, cap);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = rec[12 * i] == 1 ? new String(b, (int) outOff[i], rec[12 * i + 9], java.nio.charset.StandardCharsets.ISO_8859_1) : null;
        return res;
    }

    /**
     * GraphUtils.naiveExtend(kmers, graph, maxTipLength, minKmerCov) (src/rnabloom/util/GraphUtils.java:6935-6957) for a batch of fragments in ONE
     * native call: the left walk with the fragment's k-mers as terminators and the right walk with those and the left extension run on the device,
     * a wavefront per fragment, and nothing is written to the graph.  room is the most letters the call adds on each side of a fragment.  Returns,
     * per fragment, the string the extended list spells — the fragment itself where it is not judged (fewer than k letters, a letter other than
     * upper-case A C G T: records[16 i] == 2).  A fragment whose records[16 i] is 1 ran out of room: call again with the returned string, and with
     * phase 1 where records[16 i + 5] is not 5.  records (optional, 16 * seqs.length ints) receives the records of
     * NativeGraph.naiveExtendFragments.
     */
    public String[] naiveExtendFragments(String[] seqs, float minKmerCov, int room, int[] records) {
        return naiveExtendFragments(seqs, minKmerCov, room, null, records);
    }

    /** ... with a phase per fragment (null: all 0): 0 runs both walks, 1 the right one only */
    public String[] naiveExtendFragments(String[] seqs, float minKmerCov, int room, byte[] phase, int[] records) {
        final int n = seqs.length;
        if (phase != null && phase.length < n) throw new IllegalArgumentException("naiveExtendFragments: phase holds " + phase.length + " bytes, " + n + " are needed");
        if (records != null && records.length < 16L * n) throw new IllegalArgumentException("naiveExtendFragments: records holds " + records.length + " ints, " + 16L * n + " are needed");
        if (16L * n > Integer.MAX_VALUE) throw new IllegalArgumentException("naiveExtendFragments: " + n + " fragments' records do not fit one array: smaller batches");
        final long[] off = new long[n + 1], outOff = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("naiveExtendFragments: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        final int[] rec = records != null ? records : new int[16 * n];
        final int cap = NativeGraph.naiveExtendFragments(handle, text, off, n, phase, minKmerCov, room, outOff, null, null);
        final ByteBuffer out = ByteBuffer.allocateDirect(Math.max(cap, 1));
        NativeGraph.naiveExtendFragments(handle, text, off, n, phase, minKmerCov, room, outOff, out, rec);
        final byte[] b = new byte[cap];
        out.get(b, 0, cap);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i) res[i] = new String(b, (int) outOff[i], rec[16 * i + 4], java.nio.charset.StandardCharsets.ISO_8859_1);
        return res;
    }

    /**
     * GraphUtils.connect(ArrayList, graph, lookahead) (src/rnabloom/util/GraphUtils.java:4836-4872) for a batch of reads in ONE native call: every
     * masked stretch of every read is bridged by the six-argument getMaxCoveragePath on the device, a wavefront per gap, and the longest connected
     * run of each read is returned; nothing is written to the graph.  segments.get(i) is read i's list from SeqUtils.filterFastq / filterFasta.
     * Returns, per read, the string the reference returns, or null where it cannot be asked (an even number of entries, a segment shorter than
     * k, a letter outside ACGTU: records[8 i] == 3).  records (optional, 8 * reads ints) receives the records of NativeGraph.connectSegments.
     */
    public String[] connectSegments(java.util.List<? extends java.util.List<String>> segments, int lookahead, int[] records) {
        final int n = segments.size();
        if (records != null && records.length < 8L * n) throw new IllegalArgumentException("connectSegments: records holds " + records.length + " ints, " + 8L * n + " are needed");
        if (8L * n > Integer.MAX_VALUE) throw new IllegalArgumentException("connectSegments: " + n + " reads' records do not fit one array: smaller batches");
        final long[] readSegs = new long[n + 1], outOff = new long[n + 1];
        for (int i = 0; i < n; ++i) readSegs[i + 1] = readSegs[i] + segments.get(i).size();
        if (readSegs[n] >= Integer.MAX_VALUE) throw new IllegalArgumentException("connectSegments: too many entries in one batch");
        final long[] segOff = new long[(int) readSegs[n] + 1];
        int e = 0;
        for (java.util.List<String> list : segments) for (String s : list) { segOff[e + 1] = segOff[e] + s.length(); ++e; }
        if (segOff[e] > Integer.MAX_VALUE) throw new IllegalArgumentException("connectSegments: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) segOff[e], 1));
        for (java.util.List<String> list : segments) for (String s : list) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        final int[] rec = records != null ? records : new int[8 * n];
        final int cap = NativeGraph.connectSegments(handle, text, segOff, readSegs, n, lookahead, 1f, outOff, null, null, null);
        final ByteBuffer out = ByteBuffer.allocateDirect(Math.max(cap, 1));
        NativeGraph.connectSegments(handle, text, segOff, readSegs, n, lookahead, 1f, outOff, out, rec, null);
        final byte[] b = new byte[cap];
        out.get(b, 0, cap);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = rec[8 * i] == 3 ? null : new String(b, (int) outOff[i], rec[8 * i + 6], java.nio.charset.StandardCharsets.ISO_8859_1);
        return res;
    }

    /**
     * GraphUtils.extendRightSE (direction 0) / extendLeftSE (direction 1) (src/rnabloom/util/GraphUtils.java:6018-6204) for a batch of sequences in ONE
     * native call: the candidates' naive walks, the read-paired k-mer look-ups and the scores run on the device, a wavefront per sequence, and
     * nothing is written to the graph.  seqs are in their natural orientation, minKmerCov holds one floor per sequence.  Returns, per sequence,
     * the bases the reference's returned k-mers add, in walking order (direction 1: nearest to the sequence first), or null where the reference
     * returns null.  recs (optional, 8 * seqs.length ints) receives the records of NativeGraph.extendSE.
     */
    public String[] extendStepSE(String[] seqs, int direction, float[] minKmerCov, int[] recs) {
        final int n = seqs.length;
        if (minKmerCov.length != n) throw new IllegalArgumentException("extendStepSE: " + n + " sequences and " + minKmerCov.length + " floors");
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("extendStepSE: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        final int stride = Math.max(getReadPairedKmerDistance(), 0) + 2;
        if ((long) n * stride > Integer.MAX_VALUE || 8L * n > Integer.MAX_VALUE)
            throw new IllegalArgumentException("extendStepSE: " + n + " sequences of " + stride + " output bases do not fit one array: smaller batches");
        if (recs != null && recs.length < 8 * n) throw new IllegalArgumentException("extendStepSE: recs holds " + recs.length + " ints, " + 8 * n + " are needed");
        final byte[] bases = new byte[Math.max(n * stride, 1)];
        final int[] rec = recs != null ? recs : new int[8 * n];
        NativeGraph.extendSE(handle, text, off, n, direction, minKmerCov, bases, null, rec);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = rec[8 * i] != 0 ? new String(bases, i * stride, rec[8 * i + 3], java.nio.charset.StandardCharsets.ISO_8859_1) : null;
        return res;
    }

    /**
     * GraphUtils.extendRightPE (direction 0) / extendLeftPE (direction 1) (src/rnabloom/util/GraphUtils.java:6206-6414) for a batch of sequences in ONE
     * native call, as extendStepSE: the repeat scan, the walks, the look-ups in the read-pair and the fragment-pair filter and the scores run on
     * the device.  Returns, per sequence, the bases the reference's returned k-mers add, in walking order, or null where the reference returns
     * null (and where its isRepeat throws: recs[10 i + 1] == 5).  recs (optional, 10 * seqs.length ints) receives the records of NativeGraph.extendPE.
     */
    public String[] extendStepPE(String[] seqs, int direction, float[] minKmerCov, int[] recs) {
        final int n = seqs.length;
        if (minKmerCov.length != n) throw new IllegalArgumentException("extendStepPE: " + n + " sequences and " + minKmerCov.length + " floors");
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("extendStepPE: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        final int stride = Math.max(getFragPairedKmerDistance(), 0) + 2;
        if ((long) n * stride > Integer.MAX_VALUE || 10L * n > Integer.MAX_VALUE)
            throw new IllegalArgumentException("extendStepPE: " + n + " sequences of " + stride + " output bases do not fit one array: smaller batches");
        if (recs != null && recs.length < 10 * n) throw new IllegalArgumentException("extendStepPE: recs holds " + recs.length + " ints, " + 10 * n + " are needed");
        final byte[] bases = new byte[Math.max(n * stride, 1)];
        final int[] rec = recs != null ? recs : new int[10 * n];
        NativeGraph.extendPE(handle, text, off, n, direction, minKmerCov, bases, null, rec);
        final String[] res = new String[n];
        for (int i = 0; i < n; ++i)
            res[i] = rec[10 * i] != 0 ? new String(bases, i * stride, rec[10 * i + 3], java.nio.charset.StandardCharsets.ISO_8859_1) : null;
        return res;
    }

    public static final int SCREEN_BRANCH_FREE = 1, SCREEN_CHIMERA = 2, SCREEN_BLUNT_END = 4, SCREEN_NOT_JUDGED = 8 | 16 | 32;

    /**
     * GraphUtils.isBranchFree, isChimera and isBluntEndArtifact (src/rnabloom/util/GraphUtils.java:7651-7672, :7674-7760, :8535-8586) for a batch of
     * fragments in ONE native call, whichever of them `what` asks for (SCREEN_BRANCH_FREE | SCREEN_CHIMERA | SCREEN_BLUNT_END): the scans, the
     * gated walks and the depth searches run on the device.  assembledKmers is the worker's screeningBf — a stand-alone BloomFilter; it may be
     * null for the branch-free screen alone.  maxDepth is maxEdgeClipLength.  records (8 * seqs.length ints) receives the records of
     * NativeGraph.screenFragments: records[8 i] holds fragment i's predicates in bits 0..2, and a bit of SCREEN_NOT_JUDGED where the fragment
     * stays with the reference's own code (a letter outside ACGTU, no k-mer, a depth search past the library's budget).
     */
    public void screenFragments(String[] seqs, BloomFilter assembledKmers, int what, int lookahead, int maxDepth, int[] records) {
        final int n = seqs.length;
        if (records == null || records.length < 8L * n) throw new IllegalArgumentException("screenFragments: records must hold " + 8L * n + " ints");
        if (assembledKmers != null && (assembledKmers.getNativeWhich() != NativeGraph.DBGBF || assembledKmers.getNativeHandle() == handle))
            throw new IllegalArgumentException("screenFragments: the gate must be a stand-alone BloomFilter");
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("screenFragments: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        NativeGraph.screenFragments(handle, assembledKmers != null ? assembledKmers.getNativeHandle() : 0L, text, off, n, what, lookahead, maxDepth, 0L, records);
    }

    public static final int REPR_REPRESENTED = 1;

    /**
     * GraphUtils.represented(kmers, graph, bf, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity)
     * (src/rnabloom/util/GraphUtils.java:711-824) for a batch of sequences in ONE native call: the scan over the gate bits, the gated walks
     * and paths, the depth searches and the alignments run on the device.  screeningBf is the worker's screeningBf — a stand-alone
     * BloomFilter, required.  records (12 * seqs.length ints) receives the records of NativeGraph.represented: records[12 i] holds
     * REPR_REPRESENTED in bit 0, or a bit of SCREEN_NOT_JUDGED where the sequence stays with the reference's own code; records[12 i + 1]
     * says which line of the reference returned.
     */
    public void represented(String[] seqs, BloomFilter screeningBf, int lookahead, int maxIndelSize, int maxEdgeClipLength, float percentIdentity,
                            int[] records) {
        final int n = seqs.length;
        if (records == null || records.length < 12L * n) throw new IllegalArgumentException("represented: records must hold " + 12L * n + " ints");
        if (screeningBf == null || screeningBf.getNativeWhich() != NativeGraph.DBGBF || screeningBf.getNativeHandle() == handle)
            throw new IllegalArgumentException("represented: the gate must be a stand-alone BloomFilter");
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("represented: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        NativeGraph.represented(handle, screeningBf.getNativeHandle(), text, off, n, lookahead, maxIndelSize, maxEdgeClipLength, percentIdentity, 0L, records);
    }

    public static final int TRIM_HASHES = 0, TRIM_EDGE = 1, TRIM_LONG = 2;
    public static final int TRIM_FOUND = 1, TRIM_TRIMMED = 2, TRIM_NOT_JUDGED = 8 | 16 | 32;

    /**
     * GraphUtils.trimReverseComplementArtifact for a batch of sequences in ONE native call: mode TRIM_HASHES is
     * trimReverseComplementArtifact(kmers, graph, stranded) (src/rnabloom/util/GraphUtils.java:8588-8661), TRIM_EDGE
     * trimReverseComplementArtifact(seqKmers, maxEdgeClip, maxIndelSize, minPercentIdentity, graph) (:7918-8057) and TRIM_LONG the
     * seven-argument overload (:7762-7916); maxIndelSize and minPercentIdentity are read by neither body.  records (16 * seqs.length ints)
     * receives the records of NativeGraph.trimArtifacts: sequence i keeps the k-mers subList(records[16 i + 1], records[16 i + 2]) of its
     * getKmers list, i.e. the letters records[16 i + 1] .. records[16 i + 2] + k - 2; records[16 i] holds TRIM_FOUND where a line of the
     * reference cut (TRIM_HASHES: where the result is not null), TRIM_TRIMMED where something went, and a bit of TRIM_NOT_JUDGED where the
     * sequence stays with the reference's own code (a letter outside ACGTU, no k-mer).
     */
    public void trimReverseComplementArtifacts(String[] seqs, int mode, int maxEdgeClip, float maxCovGradient, int[] records) {
        final int n = seqs.length;
        if (records == null || records.length < 16L * n) throw new IllegalArgumentException("trimReverseComplementArtifacts: records must hold " + 16L * n + " ints");
        final long[] off = new long[n + 1];
        for (int i = 0; i < n; ++i) off[i + 1] = off[i] + seqs[i].length();
        if (off[n] > Integer.MAX_VALUE) throw new IllegalArgumentException("trimReverseComplementArtifacts: more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[n], 1));
        for (String s : seqs) for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i));
        NativeGraph.trimArtifacts(handle, text, off, n, mode, maxEdgeClip, maxCovGradient, records);
    }

    public static final int LONG_NULL = 0, LONG_UNCHANGED = 1, LONG_CHANGED = 2, LONG_NO_KMER = 3;
    public static final int LONG_OVERFLOW = 1, LONG_TRIMMED_TO_NOTHING = 2;

    /**
     * GraphUtils.correctLongSequenceWindowed (src/rnabloom/util/GraphUtils.java:3087-3185) for a batch of sequences in ONE native call (and a
     * second one for the few whose text outgrew length + 16).  Returns the strings the reference's lists spell: null where it returns null
     * (the solid-k-mer screen) or the sequence has no k-mer, "" for a list trimmed to nothing.  records (16 * seqs.length ints) receives the
     * records of NativeGraph.correctLong.
     */
    public String[] correctLongSequencesWindowed(String[] seqs, int maxErrCorrItr, float maxCovGradient, int lookahead, int maxIndelSize,
                                                 float percentIdentity, int minKmerCov, int minNumSolidKmers, boolean trimLowCovEdges,
                                                 int windowSize, int[] records) {
        final int n = seqs.length;
        if (records == null || records.length < 16L * n) throw new IllegalArgumentException("correctLongSequencesWindowed: records must hold " + 16L * n + " ints");
        final int[] params = {maxErrCorrItr, lookahead, maxIndelSize, minKmerCov, minNumSolidKmers, trimLowCovEdges ? 1 : 0, windowSize};
        final String[] result = new String[n];
        final int[] room = new int[n];
        for (int i = 0; i < n; ++i) room[i] = seqs[i].length() + 16;
        int[] todo = new int[n];
        for (int i = 0; i < n; ++i) todo[i] = i;
        for (int round = 0; round < 2 && todo.length > 0; ++round) {
            final int m = todo.length;
            final long[] off = new long[m + 1], oo = new long[m + 1];
            for (int j = 0; j < m; ++j) { off[j + 1] = off[j] + seqs[todo[j]].length(); oo[j + 1] = oo[j] + room[todo[j]]; }
            if (off[m] > Integer.MAX_VALUE || oo[m] > Integer.MAX_VALUE) throw new IllegalArgumentException("correctLongSequencesWindowed: more than 2 GB of text in one batch");
            final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[m], 1)), out = ByteBuffer.allocateDirect(Math.max((int) oo[m], 1));
            for (int j = 0; j < m; ++j) { final String s = seqs[todo[j]]; for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i)); }
            final int[] recs = new int[16 * m];
            NativeGraph.correctLong(handle, text, off, m, params, maxCovGradient, percentIdentity, oo, out, recs);
            int again = 0;
            for (int j = 0; j < m; ++j) {
                System.arraycopy(recs, 16 * j, records, 16 * todo[j], 16);
                if ((recs[16 * j + 15] & LONG_OVERFLOW) != 0) { room[todo[j]] = recs[16 * j + 2]; todo[again++] = todo[j]; continue; }
                final int status = recs[16 * j];
                if (status == LONG_NULL || status == LONG_NO_KMER) continue;
                final byte[] b = new byte[recs[16 * j + 2]];
                for (int i = 0; i < b.length; ++i) b[i] = out.get((int) oo[j] + i);
                result[todo[j]] = new String(b, java.nio.charset.StandardCharsets.ISO_8859_1);
            }
            todo = java.util.Arrays.copyOf(todo, again);
        }
        if (todo.length > 0) throw new IllegalStateException("correctLongSequencesWindowed: " + todo.length + " sequences overflowed the room their own records asked for");
        return result;
    }

    public static final int PAIRC_UNCHANGED = 0, PAIRC_CORRECTED = 1, PAIRC_NOT_JUDGED = 2;
    public static final int PAIRC_LEFT_OVERFLOW = 4, PAIRC_RIGHT_OVERFLOW = 8;

    /**
     * GraphUtils.correctErrorsPE (src/rnabloom/util/GraphUtils.java:4051-4182) for a batch of read pairs in ONE native call with every round on the
     * device (and a second one for the few mates whose text outgrew length + 16).  lefts[i] / rights[i] are replaced by the strings the reference's
     * ReadPair spells; the result is its `corrected` per pair.  A pair that is not judged (a mate without a k-mer: the reference throws) keeps its
     * texts, is reported false and has status PAIRC_NOT_JUDGED in its record.  records (16 * lefts.length ints) receives the records of
     * NativeGraph.correctPairs.  The k-mer lists are getKmers(String)'s: the worker's stretch selection comes before the call.
     */
    public boolean[] correctErrorsPE(String[] lefts, String[] rights, int lookahead, int maxIndelSize, float maxCovGradient, float covFPR,
                                     int errorCorrectionIterations, float minCovThreshold, float percentIdentity, float minKmerCov, int[] records) {
        if (lefts.length != rights.length) throw new IllegalArgumentException("correctErrorsPE: " + lefts.length + " left and " + rights.length + " right mates");
        return correctPairs(lefts, rights, new int[]{errorCorrectionIterations, lookahead, maxIndelSize},
                            new float[]{maxCovGradient, covFPR, minCovThreshold, percentIdentity, minKmerCov}, records, "correctErrorsPE");
    }

    /**
     * GraphUtils.correctErrorsSE (src/rnabloom/util/GraphUtils.java:3998-4049) for a batch of reads in ONE native call.  Returns the strings the
     * returned k-mers spell, null where the reference returns null.  records (16 * seqs.length ints) receives the records.
     */
    public String[] correctErrorsSE(String[] seqs, int lookahead, int maxIndelSize, float maxCovGradient, float covFPR, float percentIdentity,
                                    float minKmerCov, int[] records) {
        final String[] texts = seqs.clone();
        final boolean[] corrected = correctPairs(texts, null, new int[]{1, lookahead, maxIndelSize},
                                                 new float[]{maxCovGradient, covFPR, 0f, percentIdentity, minKmerCov}, records, "correctErrorsSE");
        for (int i = 0; i < texts.length; ++i) if (!corrected[i]) texts[i] = null;
        return texts;
    }

    private static ByteBuffer packText(String[] seqs, int[] todo, long[] off, String who) {
        final int m = todo.length;
        for (int j = 0; j < m; ++j) off[j + 1] = off[j] + seqs[todo[j]].length();
        if (off[m] > Integer.MAX_VALUE) throw new IllegalArgumentException(who + ": more than 2 GB of text in one batch");
        final ByteBuffer text = ByteBuffer.allocateDirect(Math.max((int) off[m], 1));
        for (int j = 0; j < m; ++j) { final String s = seqs[todo[j]]; for (int i = 0; i < s.length(); ++i) text.put((byte) s.charAt(i)); }
        return text;
    }

    private static String unpackText(ByteBuffer out, long at, int len) {
        final byte[] b = new byte[len];
        for (int i = 0; i < len; ++i) b[i] = out.get((int) at + i);
        return new String(b, java.nio.charset.StandardCharsets.ISO_8859_1);
    }

    private boolean[] correctPairs(String[] lefts, String[] rights, int[] params, float[] fparams, int[] records, String who) {
        final int n = lefts.length;
        final boolean pe = rights != null;
        if (records == null || records.length < 16L * n) throw new IllegalArgumentException(who + ": records must hold " + 16L * n + " ints");
        final boolean[] corrected = new boolean[n];
        final int[] lroom = new int[n], rroom = new int[n];
        for (int i = 0; i < n; ++i) { lroom[i] = lefts[i].length() + 16; if (pe) rroom[i] = rights[i].length() + 16; }
        int[] todo = new int[n];
        for (int i = 0; i < n; ++i) todo[i] = i;
        for (int round = 0; round < 2 && todo.length > 0; ++round) {
            final int m = todo.length;
            final long[] lo = new long[m + 1], loo = new long[m + 1], ro = pe ? new long[m + 1] : null, roo = pe ? new long[m + 1] : null;
            for (int j = 0; j < m; ++j) { loo[j + 1] = loo[j] + lroom[todo[j]]; if (pe) roo[j + 1] = roo[j] + rroom[todo[j]]; }
            if (loo[m] > Integer.MAX_VALUE || (pe && roo[m] > Integer.MAX_VALUE)) throw new IllegalArgumentException(who + ": more than 2 GB of text in one batch");
            final ByteBuffer ltext = packText(lefts, todo, lo, who), rtext = pe ? packText(rights, todo, ro, who) : null;
            final ByteBuffer lout = ByteBuffer.allocateDirect(Math.max((int) loo[m], 1)), rout = pe ? ByteBuffer.allocateDirect(Math.max((int) roo[m], 1)) : null;
            final int[] recs = new int[16 * m];
            NativeGraph.correctPairs(handle, ltext, lo, rtext, ro, m, params, fparams, loo, lout, roo, rout, recs);
            int again = 0;
            for (int j = 0; j < m; ++j) {
                final int i = todo[j];
                System.arraycopy(recs, 16 * j, records, 16 * i, 16);
                if ((recs[16 * j + 3] & (PAIRC_LEFT_OVERFLOW | PAIRC_RIGHT_OVERFLOW)) != 0) {
                    lroom[i] = Math.max(lroom[i], recs[16 * j + 4]);
                    if (pe) rroom[i] = Math.max(rroom[i], recs[16 * j + 5]);
                    todo[again++] = i;
                    continue;
                }
                corrected[i] = recs[16 * j] == PAIRC_CORRECTED;
                if (!corrected[i]) continue;
                lefts[i] = unpackText(lout, loo[j], recs[16 * j + 4]);
                if (pe) rights[i] = unpackText(rout, roo[j], recs[16 * j + 5]);
            }
            todo = java.util.Arrays.copyOf(todo, again);
        }
        if (todo.length > 0) throw new IllegalStateException(who + ": " + todo.length + " pairs overflowed the room their own records asked for");
        return corrected;
    }

    public ArrayList<Kmer> getKmers(String seq) { return getKmers(seq, 0, seq.length()); }

    public ArrayList<Kmer> getKmers(String seq, int start, int end) {
        final ArrayList<Kmer> out = new ArrayList<>();
        if (seq.length() < k) return out;
        final WindowProfile w = profile(seq, start, end);
        out.ensureCapacity(w.n);
        for (int i = 0; i < w.n; ++i) out.add(kmerAt(w, i));
        return out;
    }

    /**
     * "The longest stretch of consecutive k-mers with count >= minCoverage" as the reference computes it (:81-134), quirks included: a
     * stretch is ranked (longer wins, then the larger minimum count, then the earlier) only when a k-mer below the threshold ENDS it, and the
     * FIRST stretch is never ranked — it is what `longestSegment` points to from the start, so it is returned unless a later, ended stretch
     * takes over, and the first one that ends always does (it is compared with length 0).  A last stretch that runs to the end of the
     * sequence is returned only if it is the first.  (oracle/rbo.py::get_kmers_min_coverage is the same statement-by-statement.)
     */
    public ArrayList<Kmer> getKmers(String seq, float minCoverage) {
        final ArrayList<Kmer> out = new ArrayList<>();
        if (seq.length() < k) return out;
        final WindowProfile w = profile(seq, 0, seq.length());
        int keepAt = 0, keepLen = 0, stretches = 0, rankedLen = 0;
        float rankedMin = Float.MAX_VALUE;
        for (int i = 0; i < w.n; ) {
            if (!(w.count[i] >= minCoverage)) { ++i; continue; }
            int j = i;
            float low = Float.MAX_VALUE;
            for (; j < w.n && w.count[j] >= minCoverage; ++j) low = Math.min(low, w.count[j]);
            final int len = j - i;
            if (stretches++ == 0) { keepAt = i; keepLen = len; }
            else if (j < w.n && (len > rankedLen || (len == rankedLen && low > rankedMin))) { keepAt = i; keepLen = len; rankedLen = len; rankedMin = low; }
            i = j;
        }
        out.ensureCapacity(keepLen);
        for (int i = keepAt; i < keepAt + keepLen; ++i) out.add(kmerAt(w, i));
        return out;
    }

    // ---- k-mer lists back to sequences: all k bases of the first k-mer, then the last base of each one after it ----
    private String spell(Iterator<Kmer> kmers, int count) {
        final char[] text = new char[Math.max(count + kMinus1, 0)];
        int at = 0;
        while (kmers.hasNext()) {
            final byte[] b = kmers.next().bytes;
            if (at == 0) for (int i = 0; i < kMinus1; ++i) text[at++] = (char) b[i];
            text[at++] = (char) b[kMinus1];
        }
        return new String(text, 0, at);
    }

    private static Iterator<Kmer> backwards(final ArrayList<Kmer> list) {
        return new Iterator<Kmer>() {
            private int next = list.size() - 1;
            public boolean hasNext() { return next >= 0; }
            public Kmer next() { return list.get(next--); }
        };
    }

    public String assemble(Collection<Kmer> kmers) { return spell(kmers.iterator(), kmers.size()); }

    public String assemble(ArrayDeque<Kmer> kmers) { return spell(kmers.iterator(), kmers.size()); }

    public String assemble(ArrayList<Kmer> kmers, int start, int end) { return spell(kmers.subList(start, end).iterator(), end - start); }

    public String assembleReverseOrder(ArrayDeque<Kmer> kmers) { return spell(kmers.descendingIterator(), kmers.size()); }

    public String assembleReverseOrder(ArrayList<Kmer> kmers) { return spell(backwards(kmers), kmers.size()); }

    public byte[] assembleBytes(ArrayList<Kmer> kmers, int start, int end) {
        final byte[] text = new byte[end - start + kMinus1];
        final byte[] head = kmers.get(start).bytes;
        for (int i = 0; i < kMinus1; ++i) text[i] = head[i];
        for (int i = start; i < end; ++i) text[kMinus1 + i - start] = kmers.get(i).bytes[kMinus1];
        return text;
    }

    public byte[] assembleReverseComplementBytes(ArrayList<Kmer> kmers, int start, int end) {
        final byte[] text = assembleBytes(kmers, start, end);
        for (int lo = 0, hi = text.length - 1; lo <= hi; ++lo, --hi) {
            final byte a = complement(text[lo]), z = complement(text[hi]);
            text[lo] = z;
            text[hi] = a;
        }
        return text;
    }

    private String column(Collection<Kmer> kmers, int which) {
        final char[] text = new char[kmers.size()];
        int at = 0;
        for (Kmer kmer : kmers) text[at++] = (char) kmer.bytes[which];
        return new String(text);
    }

    public String assembleFirstBase(Collection<Kmer> kmers) { return column(kmers, 0); }

    public String assembleLastBase(Collection<Kmer> kmers) { return column(kmers, kMinus1); }

    // ---- batched forms (not in the reference): what ported hot loops call instead of n per-element calls ----
    /** op = NativeGraph.OP_*: the n base hashes are applied in array order, exactly as n per-element calls would be */
    public void applyAll(int op, long[] baseHashes, int n) { NativeGraph.apply(handle, op, baseHashes, n); }

    public void containsAll(long[] baseHashes, int n, byte[] out) { NativeGraph.contains(handle, baseHashes, n, out); }

    public void getCountAll(long[] baseHashes, int n, float[] out) { NativeGraph.getCount(handle, baseHashes, n, out); }
}
