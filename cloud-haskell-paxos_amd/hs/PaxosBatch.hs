{-# LANGUAGE ForeignFunctionInterface #-}
-- | Haskell binding of the MI355X batched Paxos engine (include/paxos_batch.h).
--
-- This is the module a maintainer adds next to the reference's src/Common.hs so
-- that app/Main.hs (/root/reference/app/Main.hs:27-53) can run batches of the
-- same single-decree protocol on GPUs instead of spawning Cloud Haskell
-- processes.  Results come back in the reference's vocabulary: 'Ticket'
-- (Common.hs:20-22), 'Command' = "c<clientId>.<t>" (Client.hs:202-203) and
-- 'Proposal' (Common.hs:29-30).
--
-- UNVERIFIED: neither this image nor the GPU box has GHC/stack/cabal
-- (SURVEY.md §8c), so this file has not been compiled.  The C side it binds is
-- exercised by tests/test_abi.py (symbols, struct layout) and the GPU tests.
--
-- The calls are `safe`: a batch blocks for the whole GPU run, and with the
-- threaded RTS (package.yaml:41-43, -threaded -with-rtsopts=-N) other
-- capabilities keep running meanwhile.
module PaxosBatch
  ( BatchConfig (..)
  , logConfig
  , Outcome (..)
  , Flag (..)
  , Totals (..)
  , defaultConfig
  , config2
  , runBatch
  , runBatchMulti
  , commandOf
    -- * Lifecycle (the host owns it: app/Main.hs start and exit)
  , abiVersion
  , initDevices
  , shutdown
  , withEngine
  , handoffCounts
    -- * Per-instance trace (the reference's `say` dumps, Server.hs:85, Client.hs:108)
  , AcceptorState (..)
  , ProposerState (..)
  , TraceStep (..)
  , traceInstance
  , TraceSel (..)
  , allSteps
  , traceBatch
    -- * Scripted schedules (the fault schedule as data: docs/SEMANTICS.md §10)
  , ScriptRows
  , scriptStride
  , scheduleExtract
  , runScripted
  , traceScripted
  , Actor (..)
  , Fate (..)
  , Message (..)
  , TraceEvent (..)
  , traceEvents
    -- * Handler-path coverage (docs/SEMANTICS.md §14)
  , CoverSummary (..)
  , CoverQuery (..)
  , coverClasses
  , cover
  , coverRange
  , ShrinkStatus (..)
  , Shrunk (..)
  , shrinkBatch
  , shrinkCoverBatch
  , Explored (..)
  , explore
  , Reach (..)
  , exploreCover
    -- * Result queries (which instances to trace, without the results on the host)
  , Query (..)
  , FlagMode (..)
  , everything
  , sweep
  ) where

import           Common                (Command, Proposal, Ticket (..))

import           Control.Exception     (bracket_)
import           Control.Monad         (forM)
import           Data.Bits             (shiftR, testBit, (.&.))
import           Data.Int              (Int32, Int64)
import           Data.Word             (Word16, Word32, Word64, Word8)
import           Foreign.C.String      (CString, peekCString)
import           Foreign.C.Types       (CInt (..))
import           Foreign.ForeignPtr    (mallocForeignPtrArray, withForeignPtr)
import           Foreign.Marshal.Array (advancePtr, allocaArray, peekArray, withArray)
import           Foreign.Marshal.Utils (with)
import           Foreign.Ptr           (Ptr, nullPtr)
import           Foreign.Storable      (Storable (..))

-- | pxb_config (72 bytes, unchanged since ABI 3, see include/paxos_batch.h).
data BatchConfig = BatchConfig
  { bcSeed          :: !Word64
  , bcFirst         :: !Word64   -- ^ global id of the first instance
  , bcCount         :: !Word64   -- ^ instances in this batch
  , bcProposers     :: !Word32   -- ^ P, clientIds 1..P  (Main.hs:45 uses 2)
  , bcAcceptors     :: !Word32   -- ^ N                  (Main.hs:41 uses 2)
  , bcLossPpm       :: !Word32
  , bcDelayMax      :: !Word32
  , bcCrashPpm      :: !Word32
  , bcCrashLenMax   :: !Word32
  , bcCrashStartMax :: !Word32
  , bcSkewMax       :: !Word32
  , bcStepCap       :: !Word32
  , bcFlags         :: !Word32
  , bcTicks         :: !Word32   -- ^ log mode: Ticks per proposer (<= 1: single decree);
                                 --   the reference ticks forever (Client.hs:96-100)
  , bcTickPeriod    :: !Word32   -- ^ steps between Ticks
  } deriving (Show)

instance Storable BatchConfig where
  sizeOf _ = 72
  alignment _ = 8
  peek p = BatchConfig
    <$> peekByteOff p 0  <*> peekByteOff p 8  <*> peekByteOff p 16
    <*> peekByteOff p 24 <*> peekByteOff p 28 <*> peekByteOff p 32
    <*> peekByteOff p 36 <*> peekByteOff p 40 <*> peekByteOff p 44
    <*> peekByteOff p 48 <*> peekByteOff p 52 <*> peekByteOff p 56
    <*> peekByteOff p 60 <*> peekByteOff p 64 <*> peekByteOff p 68
  poke p c = do
    pokeByteOff p 0  (bcSeed c);        pokeByteOff p 8  (bcFirst c)
    pokeByteOff p 16 (bcCount c);       pokeByteOff p 24 (bcProposers c)
    pokeByteOff p 28 (bcAcceptors c);   pokeByteOff p 32 (bcLossPpm c)
    pokeByteOff p 36 (bcDelayMax c);    pokeByteOff p 40 (bcCrashPpm c)
    pokeByteOff p 44 (bcCrashLenMax c); pokeByteOff p 48 (bcCrashStartMax c)
    pokeByteOff p 52 (bcSkewMax c);     pokeByteOff p 56 (bcStepCap c)
    pokeByteOff p 60 (bcFlags c);       pokeByteOff p 64 (bcTicks c)
    pokeByteOff p 68 (bcTickPeriod c)

-- | The stock topology of app/Main.hs (2 acceptors, 2 proposers), fault-free.
defaultConfig :: BatchConfig
defaultConfig = BatchConfig 0x5EED0001 0 1 2 2 0 1 0 1 0 0 256 0 1 1

-- | The stock app/Main.hs run as the reference does it: both clients keep
-- ticking (here 16 Ticks, 8 steps apart), so the acceptor logs grow.
logConfig :: BatchConfig
logConfig = defaultConfig { bcTicks = 16, bcTickPeriod = 8, bcStepCap = 1024 }

-- | BASELINE config 2: 2^20 instances, 1 proposer, 5 acceptors, no faults.
config2 :: BatchConfig
config2 = defaultConfig { bcSeed = 0x5EED0002, bcCount = 2 ^ (20 :: Int)
                        , bcProposers = 1, bcAcceptors = 5 }

data Flag = Undecided | Stuck | Panic | LogDivergence | StepCap
          | QueueOverflow | TicketOverflow | LogTrunc
  deriving (Show, Eq, Enum, Bounded)

-- | One instance's outcome (pxb_result): the Proposal of the first Execute
-- broadcast (Client.hs:178), the number of AskForTicket rounds, the steps the
-- instance ran and its flags.
data Outcome = Outcome
  { oDecided :: Maybe Proposal
  , oRounds  :: !Int
  , oSteps   :: !Int
  , oFlags   :: [Flag]
  } deriving (Show)

-- | Run totals (pxb_counters, slots of SURVEY.md §8(e)).
data Totals = Totals
  { tDecided, tUndecided, tStuck, tPanic, tDivergence, tStepCap
  , tRounds, tMessages
  , tExecutes :: !Int64           -- ^ Execute broadcasts: commands committed (log mode)
  } deriving (Show)

-- | "c<clientId>.<t>" from the command code (Client.hs:202-203).
commandOf :: Word32 -> Command
commandOf code = "c" <> show (code `shiftR` 24) <> "." <> show (code .&. 0xFFFFFF)

foreign import ccall safe "pxb_run"
  c_pxb_run :: Ptr BatchConfig -> Ptr Word32 -> Ptr Word32 -> Ptr () -> Ptr Int64 -> IO CInt
foreign import ccall safe "pxb_run_multi"
  c_pxb_run_multi :: Ptr BatchConfig -> CInt -> Ptr Word32 -> Ptr Word32 -> Ptr () -> Ptr Int64 -> IO CInt
foreign import ccall unsafe "pxb_strerror"
  c_pxb_strerror :: CInt -> IO CString
foreign import ccall unsafe "pxb_abi_version"
  c_pxb_abi_version :: IO CInt
foreign import ccall safe "pxb_init"
  c_pxb_init :: CInt -> IO CInt
foreign import ccall safe "pxb_shutdown"
  c_pxb_shutdown :: IO CInt
foreign import ccall safe "pxb_handoff_counts"
  c_pxb_handoff_counts :: CInt -> Ptr Word64 -> CInt -> IO CInt
foreign import ccall safe "pxb_trace_instance"
  c_pxb_trace_instance :: Ptr BatchConfig -> Word64 -> Ptr Word32 -> Word32 -> Ptr Word32 -> Ptr Word32 -> IO CInt

foreign import ccall safe "pxb_trace_batch"
  c_pxb_trace_batch :: Ptr BatchConfig -> Ptr Word64 -> Word64 -> Ptr Word32 -> Ptr Word32 -> Word64 -> Ptr Word64
                    -> Ptr Word32 -> Ptr Word32 -> Ptr Word64 -> IO CInt

foreign import ccall unsafe "pxb_script_stride"
  c_pxb_script_stride :: Word32 -> Word32 -> Word32 -> Word64

foreign import ccall safe "pxb_schedule_extract"
  c_pxb_schedule_extract :: Ptr BatchConfig -> Ptr Word64 -> Word64 -> Word32 -> Ptr Word8 -> IO CInt

foreign import ccall safe "pxb_run_scripted"
  c_pxb_run_scripted :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word32 -> Ptr Word32
                     -> Ptr Word32 -> Ptr Word16 -> IO CInt

foreign import ccall safe "pxb_trace_scripted"
  c_pxb_trace_scripted :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word32 -> Word64
                       -> Ptr Word64 -> Ptr Word32 -> Ptr Word32 -> Ptr Word64 -> IO CInt

foreign import ccall safe "pxb_trace_events"
  c_pxb_trace_events :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word32 -> Word64
                     -> Ptr Word64 -> Ptr Word32 -> Ptr Word32 -> Ptr Word64 -> IO CInt

foreign import ccall safe "pxb_cover"
  c_pxb_cover :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word32 -> Ptr Word32
              -> Ptr Word64 -> IO CInt

foreign import ccall safe "pxb_cover_range"
  c_pxb_cover_range :: Ptr BatchConfig -> Word64 -> Word64 -> Word64 -> Ptr Word32 -> Ptr Word64 -> Ptr Word32
                    -> Word64 -> Ptr Word64 -> IO CInt

foreign import ccall safe "pxb_shrink_batch"
  c_pxb_shrink_batch :: Ptr BatchConfig -> Ptr Word64 -> Ptr Word8 -> Word64 -> Word32 -> Word32 -> Word32
                     -> Ptr Word32 -> Ptr Word32 -> Ptr Word32 -> Ptr Word16 -> Ptr Word32 -> Ptr Word64 -> IO CInt

foreign import ccall safe "pxb_shrink_cover_batch"
  c_pxb_shrink_cover_batch :: Ptr BatchConfig -> Ptr Word64 -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32
                           -> Ptr Word32 -> Ptr Word32 -> Ptr Word32 -> Ptr Word16 -> Ptr Word32 -> Ptr Word64
                           -> Ptr Word32 -> IO CInt

foreign import ccall safe "pxb_explore"
  c_pxb_explore :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word64 -> Word64
                -> Ptr Word64 -> Ptr Word32 -> Ptr Word32 -> IO CInt

foreign import ccall safe "pxb_explore_cover"
  c_pxb_explore_cover :: Ptr BatchConfig -> Ptr Word8 -> Word64 -> Word32 -> Ptr Word32 -> Ptr Word64 -> Word64
                      -> Ptr Word64 -> Ptr Word32 -> Ptr Word32 -> Ptr Word32 -> IO CInt

foreign import ccall safe "pxb_sweep"
  c_pxb_sweep :: Ptr BatchConfig -> Ptr Word32 -> Ptr Word64 -> Ptr Word32 -> Word64 -> Ptr Word64
              -> Ptr Int64 -> Ptr Int64 -> Ptr Int64 -> IO CInt

-- | The ABI this module was written against (include/paxos_batch.h).
expectedAbi :: Int
expectedAbi = 5

-- | pxb_abi_version of the loaded library.
abiVersion :: IO Int
abiVersion = fromIntegral <$> c_pxb_abi_version

checked :: IO CInt -> IO (Either String ())
checked act = do
  rc <- act
  if rc == 0 then pure (Right ()) else Left <$> (c_pxb_strerror rc >>= peekCString)

-- | pxb_init: allocate the scratch of the first @g@ GPUs (all visible when
-- @g <= 0@) up front, at process start (where app/Main.hs:27-36 brings the
-- node up).  Optional: the first batch does it lazily.  Refuses a library
-- built for another ABI.
initDevices :: Int -> IO (Either String ())
initDevices g = do
  v <- abiVersion
  if v /= expectedAbi
    then pure (Left ("libpaxos_batch ABI " <> show v <> ", binding expects " <> show expectedAbi))
    else checked (c_pxb_init (fromIntegral g))

-- | pxb_shutdown: wait for the devices, free every scratch buffer and the
-- cached RCCL communicators (process exit).  No batch may be running on
-- another Haskell thread.
shutdown :: IO (Either String ())
shutdown = checked c_pxb_shutdown

-- | Bracket a program's batches with 'initDevices' / 'shutdown', so the
-- engine's lifetime is the host's, as the reference's node is
-- (app/Main.hs:27-53).
withEngine :: Int -> IO a -> IO (Either String a)
withEngine g body = do
  ok <- initDevices g
  case ok of
    Left err -> pure (Left err)
    Right () -> Right <$> bracket_ (pure ()) (shutdown >>= either putStrLn pure) body

-- | pxb_handoff_counts of GPU @dev@: instances the first per-lane kernel of a
-- chunk handed on, and those a second one handed on (observability only).
handoffCounts :: Int -> Bool -> IO (Either String (Word64, Word64))
handoffCounts dev reset =
  allocaArray 2 $ \p -> do
    r <- checked (c_pxb_handoff_counts (fromIntegral dev) p (if reset then 1 else 0))
    case r of
      Left err -> pure (Left err)
      Right () -> do
        [a, b] <- peekArray 2 p
        pure (Right (a, b))

-- | Run a batch on the current GPU.
runBatch :: BatchConfig -> IO (Either String ([Outcome], Totals))
runBatch cfg = runWith cfg (\pc pres ptot -> c_pxb_run pc pres nullPtr nullPtr ptot)

-- | Run a batch sharded over the first @g@ GPUs (all visible when @g <= 0@);
-- totals are all-reduced with RCCL.  Outcomes are identical to 'runBatch'.
runBatchMulti :: Int -> BatchConfig -> IO (Either String ([Outcome], Totals))
runBatchMulti g cfg =
  runWith cfg (\pc pres ptot -> c_pxb_run_multi pc (fromIntegral g) pres nullPtr nullPtr ptot)

runWith :: BatchConfig
        -> (Ptr BatchConfig -> Ptr Word32 -> Ptr Int64 -> IO CInt)
        -> IO (Either String ([Outcome], Totals))
runWith cfg call = do
  let n = fromIntegral (bcCount cfg) :: Int
  fres <- mallocForeignPtrArray (4 * n)          -- pinned: 16 B per instance
  with cfg $ \pc ->
    withForeignPtr fres $ \pres ->
      allocaArray 16 $ \ptot -> do
        rc <- call pc pres ptot
        if rc /= 0
          then Left <$> (c_pxb_strerror rc >>= peekCString)
          else do
            outs <- forM [0 .. n - 1] $ \i -> do
              [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
              pure (decode v t r f)
            tot <- peekArray 16 ptot
            let [d, u, s, p, dv, sc, rd, ms] = take 8 tot
            pure (Right (outs, Totals d u s p dv sc rd ms (tot !! 14)))

decode :: Word32 -> Word32 -> Word32 -> Word32 -> Outcome
decode v t r f = Outcome
  { oDecided = if v == 0 then Nothing
               else Just (Ticket (fromIntegral (fromIntegral t :: Int32)), commandOf v)
  , oRounds  = fromIntegral r
  , oSteps   = fromIntegral (f `shiftR` 16)
  , oFlags   = [fl | fl <- [minBound .. maxBound], testBit f (fromEnum fl)]
  }

-- | An acceptor at the end of a traced step (ServerState, Server.hs:24-31).
data AcceptorState = AcceptorState
  { asLargestTicket :: Ticket
  , asProposal      :: Maybe Proposal
  , asLogLength     :: !Int
  , asDead          :: !Bool         -- ^ after a Server.hs:76 panic (Q6)
  , asLogDigest     :: !Word32       -- ^ FNV-1a of its log so far (docs/SEMANTICS.md §7)
  } deriving (Show)

-- | A proposer at the end of a traced step (ClientState, Client.hs:58-67).
data ProposerState = ProposerState
  { psTicket     :: Ticket
  , psCommand    :: Maybe Command    -- ^ _mCommand
  , psAcks       :: !Int
  , psPhase      :: !Int             -- ^ 0 Idle, 1 Round1, 2 Round2
  , psMostRecent :: Maybe Proposal   -- ^ Round1: MostRecent
  , psRound2     :: Maybe Command    -- ^ Round2: the proposed command
  , psPending    :: !Bool            -- ^ Round2: _originalCommandPending
  } deriving (Show)

-- | One record of 'traceInstance': the state after a step (steps with nothing
-- due and no Tick change nothing and are skipped).  'tsInFlight' is Nothing
-- when copies of a broadcast were still to be sent (production variant only).
data TraceStep = TraceStep
  { tsStep      :: !Int
  , tsInFlight  :: Maybe Int
  , tsAcceptors :: [AcceptorState]
  , tsProposers :: [ProposerState]
  } deriving (Show)

-- | pxb_trace_instance: instance @i@ of @cfg@ (single decree or, ABI 5, log
-- mode) on one GPU lane, its state recorded at the end of every step, at most
-- @maxRecords@ records; with its outcome.  What 'runBatch' cannot show: where
-- a run departs from the reference's schedule, step by step.
traceInstance :: BatchConfig -> Word64 -> Int -> IO (Either String ([TraceStep], Outcome))
traceInstance cfg i maxRecords = do
  let nw = 73                                      -- sizeof(pxb_trace_step) / 4
  buf <- mallocForeignPtrArray (nw * maxRecords)
  with cfg { bcFirst = i, bcCount = 1 } $ \pc ->
    withForeignPtr buf $ \pb ->
      allocaArray 1 $ \pn ->
        allocaArray 4 $ \pres -> do
          rc <- c_pxb_trace_instance pc i pb (fromIntegral maxRecords) pn pres
          if rc /= 0
            then Left <$> (c_pxb_strerror rc >>= peekCString)
            else do
              [n] <- peekArray 1 pn
              recs <- forM [0 .. fromIntegral n - 1] $ \k -> traceStep <$> peekArray nw (advancePtr pb (nw * k))
              [v, t, r, f] <- peekArray 4 pres
              pure (Right (recs, decode v t r f))

-- | One pxb_trace_step (73 words) as a 'TraceStep'.
traceStep :: [Word32] -> TraceStep
traceStep w =
      let at k = w !! k
          nA = fromIntegral (at 2); nP = fromIntegral (at 3)
          cmd c = if c == 0 then Nothing else Just (commandOf c)
          prop t c = if c == 0 then Nothing else Just (Ticket (fromIntegral (fromIntegral t :: Int32)), commandOf c)
          acc a = let b = 4 + 4 * a; meta = at (b + 3)
                  in AcceptorState (Ticket (fromIntegral (fromIntegral (at b) :: Int32))) (prop (at (b + 1)) (at (b + 2)))
                                   (fromIntegral (meta .&. 0x7FFFFFFF)) (testBit meta 31) (at (40 + a))
          pro q = let b = 49 + 8 * q
                  in ProposerState (Ticket (fromIntegral (fromIntegral (at b) :: Int32))) (cmd (at (b + 1)))
                                   (fromIntegral (at (b + 2))) (fromIntegral (at (b + 3))) (prop (at (b + 4)) (at (b + 5)))
                                   (cmd (at (b + 6))) (at (b + 7) /= 0)
      in TraceStep (fromIntegral (at 0)) (if at 1 == 0xFFFFFFFF then Nothing else Just (fromIntegral (at 1)))
                   (map acc [0 .. nA - 1]) (map pro [0 .. nP - 1])

-- | pxb_trace_sel: which of an instance's records 'traceBatch' keeps: those
-- with a step in the inclusive range, and of those only the last 'selTail'
-- when it is not 0.
data TraceSel = TraceSel
  { selSteps :: !(Word32, Word32)
  , selTail  :: !Word32
  } deriving (Show)

-- | Every record.
allSteps :: TraceSel
allSteps = TraceSel (0, maxBound) 0

-- | pxb_trace_batch: the instances @ids@ of @cfg@ (any order, repeats allowed:
-- typically the ids a 'sweep' lists) traced in one launch, 64 per wave.  For
-- every id, in the order given: Nothing when the instance outgrew the per-lane
-- state machine's link capacities (where 'traceInstance' fails), else the
-- records the selection keeps and the instance's outcome.  Sizes the record
-- buffer with a count-only call first.
-- (additive to ABI 5: a library without the symbol fails to link)
traceBatch :: BatchConfig -> [Word64] -> TraceSel -> IO (Either String [Maybe ([TraceStep], Outcome)])
traceBatch cfg ids sel = do
  let nw = 73                                      -- sizeof(pxb_trace_step) / 4
      n = length ids
      selw = [fst (selSteps sel), snd (selSteps sel), selTail sel, 0]
      failed rc = Left <$> (c_pxb_strerror rc >>= peekCString)
  with cfg $ \pc ->
    withArray ids $ \pids ->
      withArray selw $ \psel ->
        allocaArray (n + 1) $ \poff ->
          allocaArray (max 1 n) $ \pst ->
            allocaArray (max 1 (4 * n)) $ \pres ->
              allocaArray 1 $ \ptotal -> do
                rc0 <- c_pxb_trace_batch pc pids (fromIntegral n) psel nullPtr 0 poff pst pres ptotal
                if rc0 /= 0
                  then failed rc0
                  else do
                    [total] <- peekArray 1 ptotal
                    buf <- mallocForeignPtrArray (max 1 (nw * fromIntegral total))
                    withForeignPtr buf $ \pb -> do
                      rc <- if total == 0 then pure 0
                            else c_pxb_trace_batch pc pids (fromIntegral n) psel pb total poff pst pres ptotal
                      if rc /= 0
                        then failed rc
                        else do
                          offs <- peekArray (n + 1) poff
                          sts <- peekArray n pst
                          Right <$> forM (zip3 [0 ..] (zip offs (drop 1 offs)) sts) (\(i, (o0, o1), st) ->
                            if st /= 0
                              then pure Nothing
                              else do
                                recs <- forM [fromIntegral o0 .. fromIntegral o1 - 1] $ \k ->
                                  traceStep <$> peekArray nw (advancePtr pb (nw * k))
                                [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                                pure (Just (recs, decode v t r f)))

-- | Script rows as the C ABI lays them out (include/paxos_batch.h): @count@
-- rows of 'scriptStride' bytes each, row-major.  A row is a Philox base id plus
-- overrides of its schedule draws; 0xFF / 0xFFFF fields keep what Philox gives.
type ScriptRows = [Word8]

-- | pxb_script_stride: bytes between the rows of a call of @cfg@ at @depth@.
scriptStride :: BatchConfig -> Word32 -> Int
scriptStride cfg depth = fromIntegral (c_pxb_script_stride (bcProposers cfg) (bcAcceptors cfg) depth)

-- | pxb_schedule_extract: the fully explicit rows of the schedule Philox gives
-- (seed, id), no keep anywhere.
-- (additive to ABI 5: a library without the symbol fails to link)
scheduleExtract :: BatchConfig -> [Word64] -> Word32 -> IO (Either String ScriptRows)
scheduleExtract cfg ids depth = do
  let n = length ids
      bytes = n * scriptStride cfg depth
  with cfg $ \pc ->
    withArray ids $ \pids ->
      allocaArray (max 1 bytes) $ \prows -> do
        rc <- c_pxb_schedule_extract pc pids (fromIntegral n) depth prows
        if rc /= 0 then Left <$> (c_pxb_strerror rc >>= peekCString) else Right <$> peekArray bytes prows

-- | pxb_run_scripted: @count@ rows through the per-lane state machine.  For
-- every row: Nothing when its status is not OK (beyond the link capacities, or
-- a malformed row), else its outcome and the messages sent on each link
-- (@[dirn][p][a]@ flattened: the entries of the row the run consumed).
runScripted :: BatchConfig -> ScriptRows -> Int -> Word32 -> IO (Either String [Maybe (Outcome, [Word16])])
runScripted cfg rows n depth = do
  let links = 2 * fromIntegral (bcProposers cfg) * fromIntegral (bcAcceptors cfg) :: Int
  with cfg $ \pc ->
    withArray rows $ \prows ->
      allocaArray (max 1 (4 * n)) $ \pres ->
        allocaArray (max 1 n) $ \pst ->
          allocaArray (max 1 (links * n)) $ \psent -> do
            rc <- c_pxb_run_scripted pc prows (fromIntegral n) depth pres nullPtr nullPtr pst psent
            if rc /= 0
              then Left <$> (c_pxb_strerror rc >>= peekCString)
              else do
                sts <- peekArray n pst
                Right <$> forM (zip [0 ..] sts) (\(i, st) ->
                  if st /= 0
                    then pure Nothing
                    else do
                      [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                      sent <- peekArray links (advancePtr psent (links * i))
                      pure (Just (decode v t r f, sent)))

-- | pxb_trace_scripted: 'traceBatch' with script rows in place of ids (the
-- default, end-of-step variant).
traceScripted :: BatchConfig -> ScriptRows -> Int -> Word32 -> TraceSel
              -> IO (Either String [Maybe ([TraceStep], Outcome)])
traceScripted cfg rows n depth sel = do
  let nw = 73                                      -- sizeof(pxb_trace_step) / 4
      selw = [fst (selSteps sel), snd (selSteps sel), selTail sel, 0]
      failed rc = Left <$> (c_pxb_strerror rc >>= peekCString)
  with cfg $ \pc ->
    withArray rows $ \prows ->
      withArray selw $ \psel ->
        allocaArray (n + 1) $ \poff ->
          allocaArray (max 1 n) $ \pst ->
            allocaArray (max 1 (4 * n)) $ \pres ->
              allocaArray 1 $ \ptotal -> do
                rc0 <- c_pxb_trace_scripted pc prows (fromIntegral n) depth psel nullPtr 0 poff pst pres ptotal
                if rc0 /= 0
                  then failed rc0
                  else do
                    [total] <- peekArray 1 ptotal
                    buf <- mallocForeignPtrArray (max 1 (nw * fromIntegral total))
                    withForeignPtr buf $ \pb -> do
                      rc <- if total == 0 then pure 0
                            else c_pxb_trace_scripted pc prows (fromIntegral n) depth psel pb total poff pst pres ptotal
                      if rc /= 0
                        then failed rc
                        else do
                          offs <- peekArray (n + 1) poff
                          sts <- peekArray n pst
                          Right <$> forM (zip3 [0 ..] (zip offs (drop 1 offs)) sts) (\(i, (o0, o1), st) ->
                            if st /= 0
                              then pure Nothing
                              else do
                                recs <- forM [fromIntegral o0 .. fromIntegral o1 - 1] $ \k ->
                                  traceStep <$> peekArray nw (advancePtr pb (nw * k))
                                [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                                pure (Just (recs, decode v t r f)))

-- | Who handled a message: acceptor @a@ or proposer @p@ (PXB_EVT_ACCEPTOR / _PROPOSER).
data Actor = Acceptor !Int | Proposer !Int
  deriving (Show, Eq)

-- | What became of a delivered message (PXB_EVT_HANDLED / _DISCARDED_*): a dead
-- or an isolated acceptor discards its requests; dead is told first.
data Fate = Handled | DiscardedDead | DiscardedIsolated
  deriving (Show, Eq, Enum)

-- | One message in or out of a handler (pxb_msg): a request (ClientRequest,
-- Common.hs:41-45), a response (ServerResponse, Common.hs:49-53) or the Tick.
data Message
  = AskForTicket Ticket | Propose Ticket Command | Execute Ticket
  | Round1OK Ticket (Maybe Proposal) | HaveTicket Ticket | Round2Success
  | Tick
  deriving (Show)

-- | One handler invocation (pxb_trace_event): the line the reference's `say`
-- prints after a handled message (Server.hs:85, Client.hs:108) together with
-- the messages the handler sent (the commented-out Server.hs:86, Client.hs:109).
-- 'teFrom' is the sender's index (Nothing: the ticker); 'teAfter' the actor's
-- state after the handler.
data TraceEvent = TraceEvent
  { teStep  :: !Int
  , teActor :: !Actor
  , teFrom  :: Maybe Int
  , teFate  :: !Fate
  , teIn    :: Message
  , teOut   :: [Message]
  , teAfter :: Either AcceptorState ProposerState
  } deriving (Show)

-- | One pxb_trace_event (24 words) as a 'TraceEvent'.
traceEvent :: [Word32] -> TraceEvent
traceEvent w =
      let at k = w !! k
          hdr = at 1
          isAcc = hdr .&. 0xFF == 0
          idx = fromIntegral ((hdr `shiftR` 8) .&. 0xFF) :: Int
          peer = fromIntegral ((hdr `shiftR` 16) .&. 0xFF) :: Int
          tk t = Ticket (fromIntegral (fromIntegral t :: Int32))
          cmd c = if c == 0 then Nothing else Just (commandOf c)
          prop t c = if c == 0 then Nothing else Just (tk t, commandOf c)
          request b = case at b of
            0 -> AskForTicket (tk (at (b + 1)))
            1 -> Propose (tk (at (b + 1))) (commandOf (at (b + 3)))
            _ -> Execute (tk (at (b + 1)))
          response b = case at b of
            0 -> Round1OK (tk (at (b + 1))) (prop (at (b + 2)) (at (b + 3)))
            1 -> HaveTicket (tk (at (b + 1)))
            _ -> Round2Success
          nOut = fromIntegral (at 2) :: Int
          outs = [if isAcc then response b else request b | k <- [0 .. nOut - 1], let b = 8 + 4 * k]
          meta = at 19
          after = if isAcc
            then Left (AcceptorState (tk (at 16)) (prop (at 17) (at 18)) (fromIntegral (meta .&. 0x7FFFFFFF))
                                     (testBit meta 31) (at 20))
            else Right (ProposerState (tk (at 16)) (cmd (at 17)) (fromIntegral (at 18)) (fromIntegral (at 19))
                                      (prop (at 20) (at 21)) (cmd (at 22)) (at 23 /= 0))
      in TraceEvent (fromIntegral (at 0)) (if isAcc then Acceptor idx else Proposer idx)
                    (if peer == 0xFF then Nothing else Just peer) (toEnum (fromIntegral (hdr `shiftR` 24)))
                    (if isAcc then request 4 else if at 4 == 3 then Tick else response 4) outs after

-- | pxb_trace_events: 'traceScripted' at the grain of single messages: for every
-- row Nothing when its status is not OK, else its handler events in the
-- reference model's order (docs/SEMANTICS.md §13) and its outcome.  The
-- selection's tail must be 0.  Sizes the event buffer with a count-only call
-- first.
-- (additive to ABI 5: a library without the symbol fails to link)
traceEvents :: BatchConfig -> ScriptRows -> Int -> Word32 -> TraceSel
            -> IO (Either String [Maybe ([TraceEvent], Outcome)])
traceEvents cfg rows n depth sel = do
  let nw = 24                                      -- sizeof(pxb_trace_event) / 4
      selw = [fst (selSteps sel), snd (selSteps sel), selTail sel, 0]
      failed rc = Left <$> (c_pxb_strerror rc >>= peekCString)
  with cfg $ \pc ->
    withArray rows $ \prows ->
      withArray selw $ \psel ->
        allocaArray (n + 1) $ \poff ->
          allocaArray (max 1 n) $ \pst ->
            allocaArray (max 1 (4 * n)) $ \pres ->
              allocaArray 1 $ \ptotal -> do
                rc0 <- c_pxb_trace_events pc prows (fromIntegral n) depth psel nullPtr 0 poff pst pres ptotal
                if rc0 /= 0
                  then failed rc0
                  else do
                    [total] <- peekArray 1 ptotal
                    buf <- mallocForeignPtrArray (max 1 (nw * fromIntegral total))
                    withForeignPtr buf $ \pb -> do
                      rc <- if total == 0 then pure 0
                            else c_pxb_trace_events pc prows (fromIntegral n) depth psel pb total poff pst pres ptotal
                      if rc /= 0
                        then failed rc
                        else do
                          offs <- peekArray (n + 1) poff
                          sts <- peekArray n pst
                          Right <$> forM (zip3 [0 ..] (zip offs (drop 1 offs)) sts) (\(i, (o0, o1), st) ->
                            if st /= 0
                              then pure Nothing
                              else do
                                evs <- forM [fromIntegral o0 .. fromIntegral o1 - 1] $ \k ->
                                  traceEvent <$> peekArray nw (advancePtr pb (nw * k))
                                [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                                pure (Just (evs, decode v t r f)))

-- | PXB_COVER_CLASSES: the classes of a coverage mask, bits 0 .. 28.
coverClasses :: Int
coverClasses = 29

-- | pxb_cover_summary (680 bytes: 4 + 32 + 32 words of 64 bits, 32 + 2 words of
-- 32 bits, no padding) as lists of 'coverClasses' entries, indexed by bit.
-- 'csWitness': the row index ('cover') or instance id ('coverRange') of the OK
-- row with the class that has the fewest steps, ties to the lowest i; Nothing
-- when no row has the class.
data CoverSummary = CoverSummary
  { csRowsOk       :: !Word64
  , csRowsBailed   :: !Word64
  , csRowsBad      :: !Word64
  , csMatches      :: !Word64
  , csCounts       :: [Word64]
  , csWitness      :: [Maybe Word64]
  , csWitnessSteps :: [Maybe Word32]
  , csUnion        :: !Word32
  } deriving (Show, Eq)

-- | pxb_cover_query { all_mask, any_mask, none_mask, reserved = 0 }: a row
-- matches when it is OK, has every class of 'cqAll', one of 'cqAny' (0: no
-- such condition) and none of 'cqNone'.
data CoverQuery = CoverQuery { cqAll :: !Word32, cqAny :: !Word32, cqNone :: !Word32 } deriving (Show, Eq)

coverSummaryWords :: Int
coverSummaryWords = 85                             -- sizeof(pxb_cover_summary) / 8

-- | The 85 64-bit words of a pxb_cover_summary (little-endian host).
coverSummary :: [Word64] -> CoverSummary
coverSummary w =
  let counts = take 32 (drop 4 w)
      wit = take 32 (drop 36 w)
      steps32 = concat [[fromIntegral (x .&. 0xFFFFFFFF), fromIntegral (x `shiftR` 32)] | x <- take 16 (drop 68 w)]
      has = map (/= 0) counts
      pick ok v = if ok then Just v else Nothing
  in CoverSummary (w !! 0) (w !! 1) (w !! 2) (w !! 3) (take coverClasses counts)
                  (take coverClasses (zipWith pick has wit)) (take coverClasses (zipWith pick has steps32))
                  (fromIntegral ((w !! 84) .&. 0xFFFFFFFF))

-- | pxb_cover: the coverage mask of every script row (docs/SEMANTICS.md §14):
-- per row Nothing when its status is not OK, else its mask and outcome; and the
-- call's summary, with row indices as witnesses.
-- (additive to ABI 5: a library without the symbol fails to link)
cover :: BatchConfig -> ScriptRows -> Int -> Word32 -> IO (Either String ([Maybe (Word32, Outcome)], CoverSummary))
cover cfg rows n depth =
  with cfg $ \pc ->
    withArray rows $ \prows ->
      allocaArray (max 1 n) $ \pm ->
        allocaArray (max 1 n) $ \pst ->
          allocaArray (max 1 (4 * n)) $ \pres ->
            allocaArray coverSummaryWords $ \psum -> do
              rc <- c_pxb_cover pc prows (fromIntegral n) depth pm pst pres psum
              if rc /= 0
                then Left <$> (c_pxb_strerror rc >>= peekCString)
                else do
                  ms <- peekArray n pm
                  sts <- peekArray n pst
                  summ <- coverSummary <$> peekArray coverSummaryWords psum
                  per <- forM (zip3 [0 ..] ms sts) (\(i, m, st) ->
                    if st /= 0
                      then pure Nothing
                      else do
                        [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                        pure (Just (m, decode v t r f)))
                  pure (Right (per, summ))

-- | pxb_cover_range: the coverage of the plain instances first .. first + count - 1
-- on the device, `chunk` ids at a time (0: 2^20); with a query, the first
-- maxMatches matching (id, mask) pairs in ascending order and their total in
-- 'csMatches'.  Witnesses are instance ids.  No output depends on the chunk.
coverRange :: BatchConfig -> Word64 -> Word64 -> Word64 -> Maybe CoverQuery -> Int
           -> IO (Either String (CoverSummary, [(Word64, Word32)]))
coverRange cfg first count chunk mq maxMatches =
  let nlist = maybe 0 (const maxMatches) mq
      qw = maybe [0, 0, 0, 0] (\q -> [cqAll q, cqAny q, cqNone q, 0]) mq
  in with cfg $ \pc ->
    withArray qw $ \pq ->
      allocaArray (max 1 nlist) $ \pids ->
        allocaArray (max 1 nlist) $ \pmm ->
          allocaArray coverSummaryWords $ \psum -> do
            rc <- c_pxb_cover_range pc first count chunk (maybe nullPtr (const pq) mq) pids pmm (fromIntegral nlist) psum
            if rc /= 0
              then Left <$> (c_pxb_strerror rc >>= peekCString)
              else do
                summ <- coverSummary <$> peekArray coverSummaryWords psum
                let m = min nlist (fromIntegral (csMatches summ))
                ids <- peekArray m pids
                mms <- peekArray m pmm
                pure (Right (summ, zip ids mms))

-- | What 'shrinkBatch' says of one instance (PXB_SHRINK_*).
data ShrinkStatus = ShrinkMinimal | ShrinkBudget | ShrinkNotInput | ShrinkTooMany | ShrinkUnstable
  deriving (Show, Eq, Enum)

-- | One instance of a 'shrinkBatch': its status, the faults left in its row,
-- the launches it took part in, the row's send counts (@[dirn][p][a]@
-- flattened) and outcome, and the signature of its minimal fault list (equal
-- signatures: the same minimal schedule).
data Shrunk = Shrunk
  { shStatus    :: !ShrinkStatus
  , shFaults    :: !Int
  , shLaunches  :: !Int
  , shSent      :: [Word16]
  , shOutcome   :: Outcome
  , shSignature :: !Word64
  } deriving (Show, Eq)

-- | pxb_shrink_batch: the schedules of @ids@ extracted at @depth@ and reduced to
-- 1-minimal fault sets for the predicate (flags .&. mask /= 0), all at once on
-- the device (docs/SEMANTICS.md §11); the shrunk rows and one 'Shrunk' each.
-- (additive to ABI 5: a library without the symbol fails to link)
shrinkBatch :: BatchConfig -> [Word64] -> Word32 -> Word32 -> Word32 -> IO (Either String (ScriptRows, [Shrunk]))
shrinkBatch cfg ids depth mask maxLaunches =
  fmap (\(rows, out, _) -> (rows, out)) <$>
    shrinkCall cfg ids depth (\pc pids prows n pst pnf pla psent pres psig _ ->
      c_pxb_shrink_batch pc pids prows n depth mask maxLaunches pst pnf pla psent pres psig)

-- | pxb_shrink_cover_batch: 'shrinkBatch' over a coverage predicate
-- (docs/SEMANTICS.md §16).  A run holds when it ended OK within @depth@, has one
-- of the outcome flags of @mask@ (0: no such condition) and its coverage mask
-- matches the query (as 'coverRange'; @CoverQuery 0 0 0@: any).  With the rows
-- and one 'Shrunk' each, the coverage mask of every returned row's accepted run
-- (bit index as 'coverClasses'; not an input: the given row's mask).
-- (additive to ABI 5: a library without the symbol fails to link)
shrinkCoverBatch :: BatchConfig -> [Word64] -> Word32 -> CoverQuery -> Word32 -> Word32
                 -> IO (Either String (ScriptRows, [Shrunk], [Word32]))
shrinkCoverBatch cfg ids depth (CoverQuery qAll qAny qNone) mask maxLaunches =
  withArray [mask, maxLaunches, 0, 0, qAll, qAny, qNone, 0] $ \ppred ->
    shrinkCall cfg ids depth (\pc pids prows n pst pnf pla psent pres psig pmask ->
      c_pxb_shrink_cover_batch pc pids prows n depth ppred pst pnf pla psent pres psig pmask)

-- What 'shrinkBatch' and 'shrinkCoverBatch' share: the buffers of @ids@ at
-- @depth@ around one call, and its outputs read back (the masks: zeros where
-- the call does not write them).
shrinkCall :: BatchConfig -> [Word64] -> Word32
           -> (Ptr BatchConfig -> Ptr Word64 -> Ptr Word8 -> Word64 -> Ptr Word32 -> Ptr Word32 -> Ptr Word32
               -> Ptr Word16 -> Ptr Word32 -> Ptr Word64 -> Ptr Word32 -> IO CInt)
           -> IO (Either String (ScriptRows, [Shrunk], [Word32]))
shrinkCall cfg ids depth call = do
  let n = length ids
      bytes = n * scriptStride cfg depth
      links = 2 * fromIntegral (bcProposers cfg) * fromIntegral (bcAcceptors cfg) :: Int
  with cfg $ \pc ->
    withArray ids $ \pids ->
      allocaArray (max 1 bytes) $ \prows ->
        allocaArray (max 1 n) $ \pst ->
          allocaArray (max 1 n) $ \pnf ->
            allocaArray (max 1 n) $ \pla ->
              allocaArray (max 1 (links * n)) $ \psent ->
                allocaArray (max 1 (4 * n)) $ \pres ->
                  allocaArray (max 1 n) $ \psig ->
                    withArray (replicate (max 1 n) 0) $ \pmask -> do
                      rc <- call pc pids prows (fromIntegral n) pst pnf pla psent pres psig pmask
                      if rc /= 0
                        then Left <$> (c_pxb_strerror rc >>= peekCString)
                        else do
                          rows <- peekArray bytes prows
                          sts <- peekArray n pst
                          nfs <- peekArray n pnf
                          las <- peekArray n pla
                          sigs <- peekArray n psig
                          masks <- peekArray n pmask
                          out <- forM (zip [0 ..] (zip (zip sts nfs) (zip las sigs))) $ \(i, ((st, nf), (la, sg))) -> do
                            [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                            sent <- peekArray links (advancePtr psent (links * i))
                            pure (Shrunk (toEnum (fromIntegral (st :: Word32))) (fromIntegral (nf :: Word32))
                                         (fromIntegral (la :: Word32)) sent (decode v t r f) sg)
                          pure (Right (rows, out, masks))

-- | One parent of an 'explore': whether its row was well formed, and for each
-- radius 0..3 how many of its candidates (ran OK, held, are minimal).
data Explored = Explored
  { exOk     :: !Bool
  , exCounts :: [(Int, Int, Int)]
  } deriving (Show, Eq)

-- | pxb_explore: every schedule within @radius@ (<= 3) changed link entries of
-- each of the @n@ rows, the sites being the first @siteDepth@ entries of every
-- link (docs/SEMANTICS.md §12).  Lists the candidates that hold the predicate
-- (flags .&. mask /= 0), or with @minimal@ only those of which no proper subset
-- of the changes holds, as @parent * T + c@ in ascending order, at most
-- @capacity@ of them; with them the full match count and one 'Explored' a row.
-- (additive to ABI 5: a library without the symbol fails to link)
explore :: BatchConfig -> ScriptRows -> Int -> Word32 -> Word32 -> Word32 -> Word32 -> Bool -> Int
        -> IO (Either String ([Word64], Word64, [Explored]))
explore cfg rows n depth siteDepth radius mask minimal capacity =
  with cfg $ \pc ->
    withArray rows $ \prows ->
      withArray [siteDepth, radius, mask, if minimal then 1 else 0] $ \pspace ->
        allocaArray (max 1 capacity) $ \pids ->
          allocaArray 1 $ \pn ->
            allocaArray (max 1 (12 * n)) $ \pcnt ->
              allocaArray (max 1 n) $ \pst -> do
                rc <- c_pxb_explore pc prows (fromIntegral n) depth pspace
                                    (if capacity > 0 then pids else nullPtr) (fromIntegral capacity) pn pcnt pst
                if rc /= 0
                  then Left <$> (c_pxb_strerror rc >>= peekCString)
                  else do
                    [total] <- peekArray 1 pn
                    ids <- peekArray (min capacity (fromIntegral total)) pids
                    sts <- peekArray n pst
                    out <- forM (zip [0 ..] sts) $ \(i, st) -> do
                      ws <- peekArray 12 (advancePtr pcnt (12 * i))
                      let triple r = case map fromIntegral (take 3 (drop (3 * r) ws)) of
                            [a, b, c] -> (a, b, c)
                            _         -> (0, 0, 0)
                      pure (Explored ((st :: Word32) == 0) (map triple [0 .. 3]))
                    pure (Right (ids, total, out))

-- | pxb_explore_reach of one parent (162 words): per class (bit index, as
-- 'coverClasses') the candidates that ran OK and have it at each radius 0..3,
-- and the lowest such candidate ('Nothing': none); candidate 0's mask; the
-- classes some candidate has.  The radius of 'reachFirst' is the class's reach
-- distance from the parent.
data Reach = Reach
  { reachCounts :: [[Word32]]
  , reachFirst  :: [Maybe Word32]
  , reachParent :: !Word32
  , reachUnion  :: !Word32
  } deriving (Show, Eq)

-- | pxb_explore_cover: 'explore' with the coverage classes of every candidate
-- (docs/SEMANTICS.md §15).  A candidate holds when it ran OK, has one of the
-- outcome flags of @mask@ (0: no such condition) and its coverage mask matches
-- the query (as 'coverRange'; @CoverQuery 0 0 0@: any).  Lists as 'explore'; with
-- the list one 'Explored' and one 'Reach' a row.
-- (additive to ABI 5: a library without the symbol fails to link)
exploreCover :: BatchConfig -> ScriptRows -> Int -> Word32 -> Word32 -> Word32 -> CoverQuery -> Word32
             -> Bool -> Int -> IO (Either String ([Word64], Word64, [Explored], [Reach]))
exploreCover cfg rows n depth siteDepth radius (CoverQuery qAll qAny qNone) mask minimal capacity =
  with cfg $ \pc ->
    withArray rows $ \prows ->
      withArray [siteDepth, radius, mask, if minimal then 1 else 0, qAll, qAny, qNone, 0] $ \pspace ->
        allocaArray (max 1 capacity) $ \pids ->
          allocaArray 1 $ \pn ->
            allocaArray (max 1 (12 * n)) $ \pcnt ->
              allocaArray (max 1 (162 * n)) $ \prch ->
                allocaArray (max 1 n) $ \pst -> do
                  rc <- c_pxb_explore_cover pc prows (fromIntegral n) depth pspace
                                            (if capacity > 0 then pids else nullPtr) (fromIntegral capacity) pn pcnt
                                            prch pst
                  if rc /= 0
                    then Left <$> (c_pxb_strerror rc >>= peekCString)
                    else do
                      [total] <- peekArray 1 pn
                      ids <- peekArray (min capacity (fromIntegral total)) pids
                      sts <- peekArray n pst
                      out <- forM (zip [0 ..] sts) $ \(i, st) -> do
                        ws <- peekArray 12 (advancePtr pcnt (12 * i))
                        let triple r = case map fromIntegral (take 3 (drop (3 * r) ws)) of
                              [a, b, c] -> (a, b, c)
                              _         -> (0, 0, 0)
                        pure (Explored ((st :: Word32) == 0) (map triple [0 .. 3]))
                      reach <- forM [0 .. n - 1] $ \i -> do
                        rw <- peekArray 162 (advancePtr prch (162 * i))
                        let row r = take 29 (drop (32 * r) rw)
                            firsts = [if f == maxBound then Nothing else Just f | f <- take 29 (drop 128 rw)]
                        pure (Reach (map row [0 .. 3]) firsts (rw !! 160) (rw !! 161))
                      pure (Right (ids, total, out, reach))

-- | pxb_query.flag_mode: how (flags .&. mask) is tested.
data FlagMode = AnyOf | AllOf | NoneOf
  deriving (Show, Eq, Enum)

-- | pxb_query (32 bytes): the flag test, inclusive ranges on an instance's
-- steps and rounds, and the bins of the two histograms (0: none, at most 8194;
-- values beyond the last bin are counted in it).
data Query = Query
  { qFlags      :: [Flag]
  , qMode       :: !FlagMode
  , qSteps      :: !(Word32, Word32)
  , qRounds     :: !(Word32, Word32)
  , qStepsBins  :: !Int
  , qRoundsBins :: !Int
  } deriving (Show)

-- | Matches every instance; no histograms.
everything :: Query
everything = Query [] NoneOf (0, maxBound) (0, maxBound) 0 0

-- | pxb_sweep: run the batch chunk by chunk on the current GPU and keep only
-- what the query asks for: the global ids and outcomes of the first @capacity@
-- matching instances (ascending), the number of matches, the two histograms
-- and the run totals.  Feed an id to 'traceInstance' to see what happened.
-- (additive to ABI 5: a library without the symbol fails to link)
sweep :: BatchConfig -> Query -> Int
      -> IO (Either String ([(Word64, Outcome)], Word64, [Int64], [Int64], Totals))
sweep cfg q capacity = do
  let mask = sum [2 ^ fromEnum fl | fl <- qFlags q] :: Word32
      qw = [ mask, fromIntegral (fromEnum (qMode q)), fst (qSteps q), snd (qSteps q)
           , fst (qRounds q), snd (qRounds q), fromIntegral (qStepsBins q), fromIntegral (qRoundsBins q) ]
      orNull k p = if k == 0 then nullPtr else p
  fids <- mallocForeignPtrArray (max 1 capacity)
  fres <- mallocForeignPtrArray (max 1 (4 * capacity))
  with cfg $ \pc ->
    withArray qw $ \pq ->
      withForeignPtr fids $ \pids ->
        withForeignPtr fres $ \pres ->
          allocaArray 1 $ \pn ->
            allocaArray (max 1 (qStepsBins q)) $ \phs ->
              allocaArray (max 1 (qRoundsBins q)) $ \phr ->
                allocaArray 16 $ \ptot -> do
                  rc <- c_pxb_sweep pc pq (orNull capacity pids) (orNull capacity pres) (fromIntegral capacity) pn
                                    (orNull (qStepsBins q) phs) (orNull (qRoundsBins q) phr) ptot
                  if rc /= 0
                    then Left <$> (c_pxb_strerror rc >>= peekCString)
                    else do
                      [n] <- peekArray 1 pn
                      let k = fromIntegral (min n (fromIntegral capacity)) :: Int
                      ids <- peekArray k pids
                      outs <- forM [0 .. k - 1] $ \i -> do
                        [v, t, r, f] <- peekArray 4 (advancePtr pres (4 * i))
                        pure (decode v t r f)
                      hs <- peekArray (qStepsBins q) phs
                      hr <- peekArray (qRoundsBins q) phr
                      tot <- peekArray 16 ptot
                      let [d, u, s, p, dv, sc, rd, ms] = take 8 tot
                      pure (Right (zip ids outs, n, hs, hr, Totals d u s p dv sc rd ms (tot !! 14)))
